"""The all-pairs ANY screen at pool sizes that leave partial segments, partial column groups and remainder launches.

The first stage for 13-, 14- and 15-mers is k_pairs_row (csrc/thal_pairs_row.hip kernel_body): a work item is one
row primer times a segment of up to kSegGroups = 256 column groups of 64 lanes, so a segment holds 16,384 columns of
the composition-sorted order; the last group of a pool that is not a multiple of 64 has idle lanes, and the last
segment of a pool that is not a multiple of 16,384 is short.  plan_screen (csrc/screen_plan.hpp) splits the block's rows into
launches of at most min(kChunkPairs, list_cap) = 2^29 pairs (list_cap_log2 = 29 pins the list size), in whole groups
of 24 rows, the last launch taking the remainder.  pool_sort.hip block_side picks the side of the composition blocks
the columns are sorted by: about 64 columns per block, 1 (every composition on its own) from 64 columns per
composition on.

The sizes below sit on those boundaries (segs: segments of a full-width row; tail: columns in the last segment):

    k   n        groups      segs  tail    g  launches (rows)              why
    13  35,839   559 + 63    3     3,071   2  11,952 x 2 + 11,935          one column below the switch to g = 1
    13  35,840   560         3     3,072   1  11,952 x 2 + 11,936          the switch (35,840 = 560 compositions x 64)
    13  40,001   625 + 1     3     7,233   1  13,344 x 2 + 13,313          the last group holds one lane
    13  65,503   1,023 + 31  4     16,351  1  7,296 x 8 + 7,135            the distinct headline pool (conflict cover)
    14  43,519   679 + 63    3     10,751  2  10,896 x 3 + 10,831          one column below the switch (680 x 64)
    14  43,521   680 + 1     3     10,753  1  10,896 x 3 + 10,833          one column above it
    15  52,225   816 + 1     4     3,073   1  8,712 x 5 + 8,665            one column above the switch (816 x 64)
    15  20,011   312 + 43    2     3,627   2  20,011                       two segments with the coarse sort

(groups: whole column groups + lanes of the partial one.)  test_geometry_of_the_case recomputes the table's block
sides and segment counts from restatements of the code and takes the launches from the engine's own plan
(msspe_host_screen_plan), so that the table cannot drift from what runs.
Bar, as everywhere in the suite: the oracle's decisions bit for bit, dG planes bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = -9000.0
CHUNK_PAIRS = 1 << 29          # screen_plan.hpp kChunkPairs; the engine runs with list_cap_log2 = 29
SEG_COLS = 256 * 64            # thal_pairs_row.hip kSegGroups column groups of 64 lanes
ROW_GROUP = 24                 # screen_plan.hpp kRowGroup: launches in whole row groups of 24

# name -> (k, n, block side, launches, segments)
CASES = {
    "13-35839": (13, 35839, 2, 3, 3),
    "13-35840": (13, 35840, 1, 3, 3),
    "13-40001": (13, 40001, 1, 3, 3),
    "13-65503": (13, 65503, 1, 9, 4),
    "14-43519": (14, 43519, 2, 4, 3),
    "14-43521": (14, 43521, 1, 4, 3),
    "15-52225": (15, 52225, 1, 6, 4),
    "15-20011": (15, 20011, 2, 1, 2),
}


# ---- the launch plan, and restatements of the host code that sorts the columns ------------------------------------

def launch_starts(row0: int, row1: int, ncols: int) -> list[int]:
    """First row of every launch of the block: the plan the engine executes (csrc/screen_plan.hpp plan_screen, read
    through msspe_host_screen_plan) for the row kernel under a list of 2^29 entries."""
    from msspe_amd import capi
    return capi.host_screen_plan("row", row0, row1, 0, ncols, CHUNK_PAIRS)[:, 0].tolist()


def block_side(ncols: int, k: int) -> int:
    """pool_sort.hip block_side."""
    bins = (k + 1) * (k + 2) * (k + 3) / 6.0
    g = 1
    while g < 4 and ncols / bins * g * g * g < 64.0:
        g += 1
    return g


def composition_bins(words: np.ndarray, k: int, g: int) -> np.ndarray:
    """pool_sort.hip composition_bin, over packed words (base p at bits 2p, 2p + 1)."""
    w = words.astype(np.uint64)
    base = np.stack([(w >> np.uint64(2 * p)) & np.uint64(3) for p in range(k)])
    cnt = np.stack([(base == x).sum(0) for x in range(4)]).astype(np.int64)
    b0, b1r, b2r = cnt[0] // g, cnt[1] // g, cnt[2] // g
    b1 = np.where(b0 & 1, 32 - b1r, b1r)
    b2 = np.where((b0 + b1) & 1, 32 - b2r, b2r)
    coarse = (b0 * 33 + b1) * 33 + b2
    if g == 1:
        return coarse
    f0, f1r, f2r = cnt[0] % g, cnt[1] % g, cnt[2] % g
    f1 = np.where(f0 & 1, g - 1 - f1r, f1r)
    f2 = np.where((f0 + f1) & 1, g - 1 - f2r, f2r)
    return coarse * (g * g * g) + (f0 * g + f1) * g + f2


def sorted_columns(words: np.ndarray, k: int) -> np.ndarray:
    """perm of sort_columns_by_composition over a whole pool: pool index of each sorted column (a stable sort)."""
    return np.argsort(composition_bins(words, k, block_side(len(words), k)), kind="stable")


# ---- bitmaps ------------------------------------------------------------------------------------------------------

def popcounts(bm: np.ndarray) -> np.ndarray:
    return np.bitwise_count(bm).sum(axis=1).astype(np.int64)


def unpack(bm: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(bm.view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)


def bit_column(bm: np.ndarray, c: int) -> np.ndarray:
    return ((bm[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).astype(bool)


def rebase(bm: np.ndarray, c0: int, c1: int) -> np.ndarray:
    """Columns [c0, c1) of packed rows as packed rows of their own (bit j = column c0 + j), padding bits 0."""
    nc = c1 - c0
    w = (nc + 63) // 64
    q, s = divmod(c0, 64)
    src = np.concatenate([bm, np.zeros((bm.shape[0], 1), dtype=np.uint64)], axis=1)
    out = src[:, q:q + w].copy()
    if s:
        out >>= np.uint64(s)
        out |= src[:, q + 1:q + 1 + w] << np.uint64(64 - s)
    if nc % 64:
        out[:, -1] &= np.uint64((1 << (nc % 64)) - 1)
    return out


def assert_padding_clear(bm: np.ndarray, ncols: int):
    if ncols % 64:
        pad = bm[:, -1] >> np.uint64(ncols % 64)
        assert not pad.any(), f"{int((pad != 0).sum())} rows have bits set past column {ncols}"


def bitmap_keys(bm: np.ndarray, n: int, chunk: int = 1024) -> np.ndarray:
    """Sorted row * n + column of every set bit."""
    out = []
    for r0 in range(0, bm.shape[0], chunk):
        i, j = np.nonzero(unpack(bm[r0:r0 + chunk], n))
        out.append((i + r0).astype(np.int64) * n + j)
    return np.concatenate(out)


# ---- pools, engine, screens ---------------------------------------------------------------------------------------

def make_pool(m, name: str) -> np.ndarray:
    """uint8 (n, k) ASCII.  13-65503: bench.py's headline pool with its duplicates removed, as
    test_gpu_conflict_cover.py builds it.  The others: m.synth.random_pool with three planted duplicates whose copies
    sit in the last rows and columns (the tail segment's pool columns, the last launch's rows)."""
    k, n = CASES[name][:2]
    if name == "13-65503":
        words = list(dict.fromkeys(m.synth.pool_strings(m.synth.random_pool(65536, 13))))
        assert len(words) == n
        return np.frombuffer("".join(words).encode(), dtype=np.uint8).reshape(n, k).copy()
    pool = m.synth.random_pool(n, k).copy()
    last = launch_starts(0, n, n)[-1]
    for dst, src in ((n - 1, 0), (n - 2, n // 2), (last + 1, 1)):
        pool[dst] = pool[src]
    return pool


def duplicate_groups(pool: np.ndarray) -> list[np.ndarray]:
    _, inv, cnt = np.unique(pool, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return [np.flatnonzero(inv == u) for u in np.flatnonzero(cnt > 1)]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    e.set_option("list_cap_log2", 29)      # min(kChunkPairs, list_cap) = 2^29 whatever the card's free memory
    yield e
    e.close()


def screen(eng, m, d_pool, n, k, chem, thr, rows, cols, rc0=None, want_dg=False):
    """cross_dimer_dev on the block, on the caller's stream: bitmap (started from all ones: the call clears it),
    row counts (started from rc0, or zeros) and, with want_dg, the dG plane.  Returns host arrays."""
    import torch
    (r0, r1), (c0, c1) = rows, cols
    words = (c1 - c0 + 63) // 64
    d_bm = torch.full((r1 - r0, words), -1, dtype=torch.int64, device="cuda")
    d_rc = torch.from_numpy(np.zeros(n, np.int32) if rc0 is None else rc0.astype(np.int32)).cuda()
    d_dg = torch.full((r1 - r0, c1 - c0), 7.0, dtype=torch.float64, device="cuda") if want_dg else None
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, k, chem, thr, rows, cols, d_rc.data_ptr(), d_bm.data_ptr(),
                            d_dg.data_ptr() if want_dg else 0)
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    eng.last_overflow_pairs()      # raises if a hand-over list was overrun
    out = {"bm": d_bm.cpu().numpy().view(np.uint64), "rc": d_rc.cpu().numpy().astype(np.int64),
           "dg": d_dg.cpu().numpy() if want_dg else None}
    del d_bm, d_rc, d_dg
    return out


def with_options(eng, opts: dict, fn):
    defaults = {"pair_kernel": "auto", "row_oob": 1}
    for key, v in opts.items():
        eng.set_option(key, v)
    try:
        return fn()
    finally:
        for key in opts:
            eng.set_option(key, defaults[key])


def oracle_rows(oracle, tables, pool, rows, args=None, thr=THR, want_dg=False):
    """The oracle over rows x every column, in one call: the rows are appended to the pool and screened as the
    consecutive rows [n, n + len(rows)) of the longer pool, and the appended columns are dropped."""
    n = len(pool)
    ext = np.concatenate([pool, pool[list(rows)]])
    _, dg, cf, _ = oracle.pool_pairs(tables, ext, args or oracle.ntthal_args(), thr, oracle.ANY,
                                     rows=(n, n + len(rows)), want_dg=want_dg)
    return (dg[:, :n] if want_dg else None), cf[:, :n].astype(bool)


def oracle_row_set(n: int, seed: int) -> list[int]:
    """First and last row of every launch of the full screen (rows 0 and n - 1 among them) and four seeded random
    rows."""
    starts = launch_starts(0, n, n)
    rows = set(starts) | {s - 1 for s in starts[1:]} | {n - 1}
    rows |= {int(r) for r in np.random.default_rng(seed).integers(0, n, 4)}
    return sorted(rows)


def assert_rows_equal_oracle(bm, rows, want, n, what):
    got = unpack(bm[rows], n)
    bad = [(r, np.flatnonzero(got[i] != want[i])) for i, r in enumerate(rows) if (got[i] != want[i]).any()]
    assert not bad, f"{what}: {len(bad)} of {len(rows)} rows differ from the oracle; " + "; ".join(
        f"row {r}: {c.size} columns, first {c[:5].tolist()}" for r, c in bad[:4])


def check_full_screen(pool, out, rc0, stats):
    """Counts added to rc0 are the row popcounts, padding bits are 0, no replay mismatch in either stage, and
    duplicate oligos give equal rows and equal columns."""
    n = len(pool)
    bm = out["bm"]
    assert bm.shape == (n, (n + 63) // 64)
    pop = popcounts(bm)
    np.testing.assert_array_equal(out["rc"] - rc0, pop)
    assert_padding_clear(bm, n)
    assert stats["replay_mismatch"] == 0 and stats["list"]["replay_mismatch"] == 0, stats
    assert 0 < pop.sum() < n * n // 4
    for grp in duplicate_groups(pool):
        for j in grp[1:]:
            np.testing.assert_array_equal(bm[j], bm[grp[0]], err_msg=f"rows {grp[0]} and {j}: the same oligo")
            np.testing.assert_array_equal(bit_column(bm, int(j)), bit_column(bm, int(grp[0])),
                                          err_msg=f"columns {grp[0]} and {j}: the same oligo")


# ---- one pool per case, screened once ------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=list(CASES))
def case(request, m, eng):
    """The case's pool on the device and its full decisions-only screen (bitmap and counts, no planes), from a
    bitmap of ones and nonzero counts."""
    import torch
    name = request.param
    k, n = CASES[name][:2]
    pool = make_pool(m, name)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    rc0 = (np.arange(n, dtype=np.int64) * 7919) % 1000 + 1
    eng.pair_stage_stats()
    out = screen(eng, m, d_pool, n, k, m.Chem.ntthal(), THR, (0, n), (0, n), rc0=rc0)
    stats = eng.pair_stage_stats()
    c = {"name": name, "k": k, "n": n, "pool": pool, "d_pool": d_pool, "out": out, "rc0": rc0, "stats": stats}
    yield c
    del c["d_pool"], c["out"]
    torch.cuda.empty_cache()


def test_geometry_of_the_case(case, eng):
    """The module docstring's table from the engine's plan and the restated sort; the row kernel is the first stage."""
    k, n, g, n_launch, n_seg = CASES[case["name"]]
    assert block_side(n, k) == g
    starts = launch_starts(0, n, n)
    assert len(starts) == n_launch
    assert ((n + 63) // 64 + 255) // 256 == n_seg >= 2
    assert n % SEG_COLS                      # a short tail segment
    if n_launch > 1:
        rows = starts[1]
        assert rows % ROW_GROUP == 0 and rows * n <= CHUNK_PAIRS and n - starts[-1] < rows   # a remainder at the end
    assert eng.info("row_kernel") == 1


def test_full_screen_counts_padding_and_duplicates(case):
    """The full decisions-only screen of the case: counts, padding bits, replay, duplicate rows and columns."""
    check_full_screen(case["pool"], case["out"], case["rc0"], case["stats"])
    if case["name"] != "13-65503":
        assert len(duplicate_groups(case["pool"])) >= 3


def test_launch_edge_rows_equal_the_oracle(case, oracle, oracle_tables):
    """Whole rows (the tail segment and its partial group included) against the oracle: the first and last row of
    every launch, rows 0 and n - 1, four seeded random rows."""
    n = case["n"]
    rows = oracle_row_set(n, seed=n)
    _, want = oracle_rows(oracle, oracle_tables, case["pool"], rows)
    assert_rows_equal_oracle(case["out"]["bm"], rows, want, n, case["name"])


def test_other_first_stages_agree(case, eng, m):
    """13-mers: the f64 register-table first stage (pair_kernel = f64) and the general integer kernel (row_oob = 0),
    whose blocks and launches are shaped otherwise, give the whole bitmap and the counts bit for bit.  14- and
    15-mers: the general integer kernel (pair_kernel = int) on the whole matrix, and the f64 first stage on a row
    block of 300 rows across the full screen's first launch boundary."""
    k, n, d_pool = case["k"], case["n"], case["d_pool"]
    bm, pop = case["out"]["bm"], popcounts(case["out"]["bm"])
    chem = m.Chem.ntthal()

    def run(rows=(0, n)):
        assert eng.info("row_kernel") == 0
        return screen(eng, m, d_pool, n, k, chem, THR, rows, (0, n))

    for opts in ([{"pair_kernel": "f64"}, {"row_oob": 0}] if k == 13 else [{"pair_kernel": "int"}]):
        other = with_options(eng, opts, run)
        bad = (other["bm"] != bm).any(1)
        assert not bad.any(), f"{opts}: {int(bad.sum())} rows differ, first {np.flatnonzero(bad)[:5]}"
        np.testing.assert_array_equal(other["rc"], pop)
        del other
    if k != 13:
        starts = launch_starts(0, n, n)
        b = starts[1] if len(starts) > 1 else n - 150
        r0, r1 = b - 150, min(n, b + 150)
        other = with_options(eng, {"pair_kernel": "f64"}, lambda: run((r0, r1)))
        np.testing.assert_array_equal(other["bm"], bm[r0:r1])
        np.testing.assert_array_equal(other["rc"][r0:r1], pop[r0:r1])
        assert not other["rc"][:r0].any() and not other["rc"][r1:].any()


def test_column_blocks_with_unaligned_edges(case, eng, m):
    """Blocks (0, 16,383), (16,383, 16,385), (16,385, n) and (n - 1, n) of every row, and of a 600-row block whose
    row0 is no multiple of 24: each block's bits, rebased to its col0, are the full bitmap's slice; counts of rows
    outside the block stay 0."""
    k, n, d_pool = case["k"], case["n"], case["d_pool"]
    bm = case["out"]["bm"]
    starts = launch_starts(0, n, n)
    r0 = starts[1] - 301 if len(starts) > 1 else 1237
    assert r0 % ROW_GROUP
    for rows in ((0, n), (r0, r0 + 600)):
        for cols in ((0, SEG_COLS - 1), (SEG_COLS - 1, SEG_COLS + 1), (SEG_COLS + 1, n), (n - 1, n)):
            out = screen(eng, m, d_pool, n, k, m.Chem.ntthal(), THR, rows, cols)
            want = rebase(bm[rows[0]:rows[1]], *cols)
            bad = (out["bm"] != want).any(1)
            assert not bad.any(), f"rows {rows} cols {cols}: {int(bad.sum())} rows differ, first {np.flatnonzero(bad)[:5]}"
            rc = np.zeros(n, dtype=np.int64)
            rc[rows[0]:rows[1]] = popcounts(want)
            np.testing.assert_array_equal(out["rc"], rc, err_msg=f"rows {rows} cols {cols}")


def test_shuffled_pool_gives_the_permuted_bitmap(case, eng, m):
    """A seeded shuffle p of the pool: bit (i, j) of its screen is bit (p[i], p[j]) of the original's, and its counts
    are the original's permuted (a write-back through the wrong perm entry of the composition sort shows here)."""
    import torch
    k, n = case["k"], case["n"]
    p = np.random.default_rng(n + k).permutation(n)
    d_pool = torch.from_numpy(m.pack_oligos(case["pool"][p]).view(np.int64)).cuda()
    out = screen(eng, m, d_pool, n, k, m.Chem.ntthal(), THR, (0, n), (0, n))
    np.testing.assert_array_equal(out["rc"], popcounts(case["out"]["bm"])[p])
    shifts = torch.arange(8, dtype=torch.uint8, device="cuda")

    def bits(words):      # packed rows (host) -> (r, n) 0/1 bytes on the device
        b = torch.from_numpy(np.ascontiguousarray(words).view(np.uint8)).cuda()
        return ((b.unsqueeze(-1) >> shifts) & 1).reshape(b.shape[0], -1)[:, :n]

    d_p = torch.from_numpy(p).cuda()
    for i0 in range(0, n, 2048):
        i1 = min(n, i0 + 2048)
        want = bits(case["out"]["bm"][p[i0:i1]])[:, d_p]
        diff = (bits(out["bm"][i0:i1]) != want).any(1)
        assert not bool(diff.any()), f"{int(diff.sum())} shuffled rows in [{i0}, {i1}) differ"


# ---- 40,001 13-mers: edge lists and dG planes --------------------------------------------------------------------

@pytest.fixture(scope="module")
def odd(m, eng):
    import torch
    pool = make_pool(m, "13-40001")
    n = len(pool)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    out = screen(eng, m, d_pool, n, 13, m.Chem.ntthal(), THR, (0, n), (0, n))
    yield {"pool": pool, "n": n, "d_pool": d_pool, "bm": out["bm"]}
    torch.cuda.empty_cache()


def test_edges_are_the_set_bits_at_40001(odd, eng, m):
    """The host edge list of the whole pool: too small a capacity is MSSPE_ERR_CAPACITY with the true count; then
    the edges, in row-major order, are exactly the bitmap's set bits."""
    pool, n, bm = odd["pool"], odd["n"], odd["bm"]
    total = int(popcounts(bm).sum())
    with pytest.raises(m.MsspeError) as err:
        eng.cross_dimer_edges(pool, m.Chem.ntthal(), THR, capacity=total - 1)
    assert m.STATUS[err.value.code] == "MSSPE_ERR_CAPACITY" and err.value.count == total
    edges, count = eng.cross_dimer_edges(pool, m.Chem.ntthal(), THR, capacity=total)
    assert count == total
    keys = edges["a"].astype(np.int64) * n + edges["b"].astype(np.int64)
    np.testing.assert_array_equal(keys, bitmap_keys(bm, n))


# rows 13,339 .. 13,350: row0 and row1 no multiple of 24, across the full screen's first launch boundary (13,344)
DG_ROWS = (13339, 13351)


def test_dg_block_and_own_value_cuts_at_40001(odd, eng, m, oracle, oracle_tables):
    """A dG row block with unaligned row0 / row1 and every column: the oracle's dG bit for bit, its bits and the full
    screen's.  Then thresholds that are the block's own pairs' dG in the tail segment of the composition-sorted
    columns (the pair in the last group's single lane first): decisions with planes and without are the oracle's
    plane cut."""
    pool, n, d_pool, bm = odd["pool"], odd["n"], odd["d_pool"], odd["bm"]
    r0, r1 = DG_ROWS
    assert r0 % ROW_GROUP and r1 % ROW_GROUP and r0 < launch_starts(0, n, n)[1] < r1
    dg, cf = oracle_rows(oracle, oracle_tables, pool, list(range(r0, r1)), want_dg=True)
    chem = m.Chem.ntthal()
    out = screen(eng, m, d_pool, n, 13, chem, THR, (r0, r1), (0, n), want_dg=True)
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(unpack(out["bm"], n), cf)
    np.testing.assert_array_equal(out["bm"], bm[r0:r1])
    np.testing.assert_array_equal(out["rc"][r0:r1], cf.sum(1))

    perm = sorted_columns(m.pack_oligos(pool), 13)
    tail = perm[2 * SEG_COLS:]                       # the third segment's columns, in sorted order
    picks = []
    for c in (int(tail[-1]), int(tail[0]), int(tail[tail.size // 2])):   # the last lane, the tail's first and middle
        finite = np.flatnonzero(np.isfinite(dg[:, c]))
        if finite.size:
            picks.append((int(finite[0]), c))
    assert picks and picks[0][1] == int(tail[-1]), "no pair of the block in the last lane has a structure"
    for i, c in picks:
        thr = float(np.float32(dg[i, c]))
        want = dg <= m.g_cut(thr)
        planes = screen(eng, m, d_pool, n, 13, chem, thr, (r0, r1), (0, n), want_dg=True)
        fast = screen(eng, m, d_pool, n, 13, chem, thr, (r0, r1), (0, n))
        np.testing.assert_array_equal(planes["dg"], dg)
        for what, got in (("with planes", planes), ("decisions only", fast)):
            np.testing.assert_array_equal(unpack(got["bm"], n), want, err_msg=f"{what}, cut at pair ({r0 + i}, {c})")
            np.testing.assert_array_equal(got["rc"][r0:r1], want.sum(1), err_msg=what)


# ---- one non-default chemistry -----------------------------------------------------------------------------------

def test_primer3_chemistry_at_35839(m, eng, oracle, oracle_tables):
    """Primer3's chemistry on the 13-mer pool one column below the sort's switch: the full screen's counts, padding,
    replay and duplicates, and the launch-edge, end and random rows against the oracle."""
    import torch
    pool = make_pool(m, "13-35839")
    n = len(pool)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    rc0 = np.full(n, 3, dtype=np.int64)
    eng.pair_stage_stats()
    out = screen(eng, m, d_pool, n, 13, m.Chem.primer3(), THR, (0, n), (0, n), rc0=rc0)
    check_full_screen(pool, out, rc0, eng.pair_stage_stats())
    rows = oracle_row_set(n, seed=3 * n)
    _, want = oracle_rows(oracle, oracle_tables, pool, rows, args=oracle.p3_args())
    assert_rows_equal_oracle(out["bm"], rows, want, n, "primer3")
