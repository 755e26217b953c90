"""The split rule of the thal-scored site passes (csrc/slab_split.hpp, read through msspe_host_slab_split: no GPU)
against the Python model of tests/slab_split_model.py, part for part, and the invariants the slab loop (capi.cpp
run_slabs) relies on, checked on the parts themselves: they tile the slab on the axis that was cut and leave the other
alone, none is empty, a slab that can be cut gives at least two (count > cap makes ceil(2 count / cap) >= 3), the outer
axis is cut before the primers, and only one outer element against one primer cannot be split."""
import numpy as np
import pytest

from slab_split_model import slab_split_model

O0, O1, P0, P1 = range(4)


@pytest.fixture(scope="module")
def split():
    from msspe_amd import capi
    return capi.host_slab_split


def slabs():
    """(o0, o1, p0, p1, count, cap) with count > cap: seeded, then the corners."""
    rng = np.random.default_rng(20261)
    out = []

    def add(outer, prim, count, cap, o0=None, p0=None):
        o0 = int(rng.integers(0, 1 << 31)) if o0 is None else o0
        p0 = int(rng.integers(0, 100000)) if p0 is None else p0
        out.append((o0, o0 + outer, p0, p0 + prim, count, cap))

    for _ in range(3000):
        cap = int(rng.integers(2, (1 << 22) + 1)) if rng.integers(0, 2) else 1 << int(rng.integers(1, 23))
        # counts from just above the list to 2^40, evenly over the magnitudes
        count = min(1 << 40, cap + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 41)))))
        outer, prim = (int(x) if rng.integers(0, 4) else 1 for x in rng.integers(1, 5001, 2))
        add(outer, prim, count, cap)
    for cap in (2, 3, 4096, (1 << 22) - 1, 1 << 22):
        for count in (cap + 1, 2 * cap, 2 * cap + 1, 7 * cap // 2, 1 << 40):      # want = 3, 4, 5, 7 and far above
            for outer, prim in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 5000), (5000, 1), (5000, 5000), (3, 4), (6, 1), (1, 6)):
                add(outer, prim, count, cap)
                add(outer, prim, count, cap, o0=0, p0=0)
                add(outer, prim, count, cap, o0=(1 << 31) - 1)
    return out


def test_parts_equal_the_model_and_tile_the_slab(split):
    seen = {"outer": 0, "primers": 0, "none": 0, "want above the extent": 0}
    for o0, o1, p0, p1, count, cap in slabs():
        what = f"[{o0}, {o1}) x [{p0}, {p1}) count {count} cap {cap}"
        parts = split(o0, o1, p0, p1, count, cap)
        assert parts.tolist() == [list(p) for p in slab_split_model(o0, o1, p0, p1, count, cap)], what
        if o1 - o0 == 1 and p1 - p0 == 1:
            assert len(parts) == 0, what                       # cannot be split: exactly here
            seen["none"] += 1
            continue
        assert len(parts) >= 2, what
        lo, hi, same = (O0, O1, (P0, P1)) if o1 - o0 > 1 else (P0, P1, (O0, O1))      # the outer axis first
        seen["outer" if lo == O0 else "primers"] += 1
        start, end = (o0, o1) if lo == O0 else (p0, p1)
        assert parts[0, lo] == start and parts[-1, hi] == end and (parts[1:, lo] == parts[:-1, hi]).all(), what
        assert (parts[:, hi] > parts[:, lo]).all(), what                                # no part is empty
        assert (parts[:, same] == ((p0, p1) if lo == O0 else (o0, o1))).all(), what     # the other axis as it was
        want = -(-2 * count // cap)
        assert len(parts) == min(end - start, want), what
        seen["want above the extent"] += want > end - start
    assert all(n >= 20 for n in seen.values()), seen


def test_pinned_splits(split):
    # a list of 2^12 overrun by 5,000 matches: three parts; 24 groups, then one group's 130 primers
    assert split(0, 24, 0, 130, 5000, 4096).tolist() == [[0, 8, 0, 130], [8, 16, 0, 130], [16, 24, 0, 130]]
    assert split(7, 8, 0, 130, 5000, 4096).tolist() == [[7, 8, 0, 43], [7, 8, 43, 86], [7, 8, 86, 130]]
    assert split(0, 10, 5, 6, 4097, 4096).tolist() == [[0, 3, 5, 6], [3, 6, 5, 6], [6, 10, 5, 6]]      # count == cap + 1
    assert split(0, 2, 0, 9, 1 << 40, 2).tolist() == [[0, 1, 0, 9], [1, 2, 0, 9]]                       # want above the extent
    assert split(3, 4, 8, 9, 4196, 4096).tolist() == []


def test_what_the_hook_refuses(split):
    import ctypes as C

    import msspe_amd
    for args in ((0, 0, 0, 5, 10, 4), (5, 4, 0, 5, 10, 4), (-1, 4, 0, 5, 10, 4), (0, 4, 5, 5, 10, 4), (0, 4, -1, 5, 10, 4),
                 (0, 4, 0, 5, 10, 0), (0, 4, 0, 5, 4, 4), (0, 4, 0, 5, 3, 4), (0, 1 << 32, 0, 5, 10, 4),
                 (0, 4, 0, 5, 1 << 63, 4)):
        with pytest.raises(msspe_amd.MsspeError) as e:
            split(*args)
        assert e.value.code == 1, args                                                  # MSSPE_ERR_ARG
    # the capacity / n_out convention of msspe_host_screen_plan: too small a buffer writes nothing and says how many
    L, n, out = msspe_amd.load_library(), C.c_int(-1), np.full((2, 4), -7, dtype=np.int64)
    assert L.msspe_host_slab_split(0, 24, 0, 130, 5000, 4096, out.ctypes.data, 2, C.byref(n)) == 5 and n.value == 3
    assert (out == -7).all()
    assert L.msspe_host_slab_split(0, 24, 0, 130, 5000, 4096, None, 0, C.byref(n)) == 5 and n.value == 3
    assert L.msspe_host_slab_split(0, 24, 0, 130, 5000, 4096, None, 3, C.byref(n)) == 1
    assert L.msspe_host_slab_split(0, 24, 0, 130, 5000, 4096, out.ctypes.data, 2, None) == 1
