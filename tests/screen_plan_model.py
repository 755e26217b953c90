"""A Python model of csrc/screen_plan.hpp: how a pair screen's block is cut into first-stage launches and where the
hand-over lists are flushed.  Written from the rules, not from the header's loops (cumulative sums and a sorted search
where the header bisects), so that tests/test_screen_plan_model.py compares two statements of the same geometry.

A launch is (row0, row1, col0, col1, pairs, list_entries, flush_before), the columns of msspe_host_screen_plan."""
import numpy as np

CHUNK_PAIRS = 1 << 29      # most pairs of one launch
ROW_GROUP = 24             # launches other than a block's last cover whole groups of 24 rows
FIRST_STAGES = ("dense", "wave", "split", "fast", "int", "row", "bound", "bound_mirror")


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def rows_per_launch(n_rows: int, ncols: int, list_cap: int) -> int:
    """The rectangular and the dense rule: the block's rows spread evenly over as few launches of at most
    min(CHUNK_PAIRS, list_cap) pairs as possible, rounded up to whole row groups but never past the largest
    whole-group launch; a row longer than a launch is a launch band of its own."""
    max_rows = max(1, min(CHUNK_PAIRS, list_cap) // ncols)
    if n_rows <= max_rows:
        return n_rows
    largest = max_rows // ROW_GROUP * ROW_GROUP if max_rows > ROW_GROUP else max_rows
    rows = ceil_div(n_rows, ceil_div(n_rows, largest))
    return min(largest, ceil_div(rows, ROW_GROUP) * ROW_GROUP) if rows > ROW_GROUP else rows


def mirrored_ranges(n: int, list_cap: int) -> list[tuple[int, int, int]]:
    """The mirrored rule: sorted rows [p0, p1) of a square block of n, row p screening the n - p columns from itself on,
    cut into launches of near-equal pair counts within min(CHUNK_PAIRS, list_cap // 2): (p0, p1, pairs)."""
    cap = min(CHUNK_PAIRS, list_cap // 2)
    done = np.concatenate([[0], np.cumsum(n - np.arange(n, dtype=np.int64))])     # done[p]: pairs of rows [0, p)
    total = int(done[n])
    target = ceil_div(total, ceil_div(total, cap))
    out, p0 = [], 0
    while p0 < n:
        first = int(np.searchsorted(done, done[p0] + target, side="left"))        # the first p1 that reaches the target
        first = min(max(first, p0 + 1), n)
        p1 = min(n, p0 + ceil_div(first - p0, ROW_GROUP) * ROW_GROUP)
        while p1 > p0 + 1 and done[p1] - done[p0] > cap:
            p1 -= 1
        out.append((p0, p1, int(done[p1] - done[p0])))
        p0 = p1
    return out


def screen_plan_model(first_stage: str, row0: int, row1: int, col0: int, ncols: int, list_cap: int) -> np.ndarray:
    """int64 (launches, 7), as capi.host_screen_plan returns it."""
    assert first_stage in FIRST_STAGES
    if first_stage == "bound_mirror":
        assert row0 == col0 and row1 - row0 == ncols and ncols <= min(CHUNK_PAIRS, list_cap // 2)
        cells = [(p0, p1, 0, ncols, pairs, 2 * pairs) for p0, p1, pairs in mirrored_ranges(ncols, list_cap)]
    else:
        step = rows_per_launch(row1 - row0, ncols, list_cap)
        chunk = min(CHUNK_PAIRS, list_cap)
        cells = []
        for r in range(row0, row1, step):
            rows = min(row1, r + step) - r
            if first_stage == "dense":            # a band of rows over every column; nothing is handed on
                cells.append((r, r + rows, col0, col0 + ncols, rows * ncols, 0))
                continue
            base = col0 if first_stage == "wave" else 0      # pool columns / positions in the sorted order
            for q in range(0, ncols, chunk):
                cols = min(ncols, q + chunk) - q
                cells.append((r, r + rows, base + q, base + q + cols, rows * cols, rows * cols))
    plan, pending = [], 0
    for cell in cells:
        flush = pending + cell[5] > list_cap
        pending = cell[5] if flush else pending + cell[5]
        plan.append(cell + (int(flush),))
    return np.asarray(plan, dtype=np.int64).reshape(-1, 7)
