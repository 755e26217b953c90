"""The generated packed scan run in an interpreter, without a GPU (tools/gen_row_bound_packed_asm.py, no argument;
tests/scan_interpreter.py).

The scan of k_pairs_bound_packed (row_bound_packed_pinned.inc) issues every chunk's table reads before the chunk in
front of it is reduced and waits by count; the chunk that straddles rows i-2 / i-1 and the chunks of row i-1 leave the
straight line.  A missing or miscounted wait gives silently wrong minima on the device; here the interpreter delivers
every LDS value at the last moment its wait allows and raises when a register is used or overwritten while its read is
outstanding.

For every (NFAR, NEAR, NRUN) the kernel can pass -- every (first slot of row i-1, of row i) with rows up to 13 wide in
a table of up to 52 slots; the scan always enters at chunk 0 -- random slot words and a random table (a third of its
entries "not available"): the two accumulators == the direct formula over the visited slots.  (The ring scans of the
windowed instance: tests/test_pair_bound_ring_model.py; this file is the generator's output:
tests/test_pair_bound_packed_model.py.)"""
import random

import pytest

from scan_interpreter import ROOT, Hazard, Program, s32, scan_lines

CSRC = ROOT / "open-msspe-design_amd" / "csrc"
KC, NS, W0 = 4, 52, 76
OFF = 1 << 28


@pytest.fixture(scope="module")
def single():
    return Program(scan_lines((CSRC / "row_bound_packed_pinned.inc").read_text()))


def controls():
    """Every distinct (0, NFAR, NEAR, NRUN) run_pair_packed can pass: s1 <= r the first slots of rows i-1, i."""
    seen = set()
    for s1 in range(NS + 1):
        for r in range(s1, min(s1 + 13, NS) + 1):
            seen.add((0, s1 // KC, s1, (r + KC - 1) // KC))
    return sorted(seen)


def make_case(rng):
    """Slot words K << 17 | field (bits 15, 16 zero), two cells' minuends above every K, cell-side terms (one of them
    the void 1 << 26 now and then), and a table word per byte address: 0 (not available) or OFF - entry."""
    words = [(rng.randrange(0, 900) << 17) | rng.randrange(0, 0x8000) for _ in range(NS)]
    cells = [(((rng.randrange(900, 4000)) << 17) | 0x7fff, rng.choice([rng.randrange(-3000, 3000), 1 << 26])) for _ in range(2)]
    seed = rng.randrange(1 << 30)

    def table(addr, area="TOFF"):
        assert area == "TOFF" and addr % 4 == 0 and 0 <= addr < (4000 << 2) + 4, addr
        x = random.Random(seed * 8191 + addr)
        return 0 if x.random() < 1 / 3 else OFF - x.randrange(-40000, 40000)

    return words, cells, table


def formula(words, C, Y, table, start, nfar, near, nrun):
    far = nr = 0
    for s in range(start * KC, min(nrun * KC, NS)):
        pc = s // KC
        t = (C - words[s]) & 0xffffffff
        cand = s32((t & 0xffff) + table(t >> 15))
        if nfar > pc:
            far = max(far, cand)
        else:
            if near > pc * KC and near > s:      # the straddling chunk: slots of rows i-2 and above take the cell-side term
                cand = s32(cand - Y)
            nr = max(nr, cand)
    return far & 0xffffffff, nr & 0xffffffff


def run_single(prog, words, C, Y, table, ctl):
    start, nfar, near, nrun = ctl
    assert start == 0
    v = {f"v{W0 + s}": w for s, w in enumerate(words)}
    v.update({"%[C]": C, "%[Y]": Y & 0xffffffff})
    out = prog.run(v, {"%[NFAR]": nfar, "%[NEAR]": near, "%[NRUN]": nrun}, table)
    assert [out[f"v{W0 + s}"] for s in range(NS)] == words      # the slot table is read only
    return out["v74"], out["v75"]


def test_single_scan_equals_the_formula_under_counted_waits(single):
    rng = random.Random(6100)
    ctls = controls()
    ran, kinds = 0, set()
    for ctl in ctls:
        words, cells, table = make_case(rng)
        C, Y = cells[0]
        got = run_single(single, words, C, Y, table, ctl)
        assert got == formula(words, C, Y, table, *ctl), ctl
        _, nfar, near, nrun = ctl
        ran += nrun > 0
        for pc in range(nrun):
            kinds.add(("far" if nfar > pc else "straddle" if near > pc * KC else "near", pc + 1 < nrun))
    assert len(ctls) == 198 and ran >= 190
    # every chunk kind with and without a chunk behind it
    assert kinds == {(kind, nxt) for kind in ("far", "straddle", "near") for nxt in (False, True)}


def test_interpreter_finds_a_wrong_wait(single):
    """The check has teeth: every reached wait, made to count one read too many, raises Hazard (the interpreter delivers a
    value at the last moment its wait allows, so the chunk's last read is still outstanding where it is used)."""
    rng = random.Random(6300)
    words, cells, table = make_case(rng)
    prog = single
    waits = [i for i, (name, a) in enumerate(prog.ops) if name == "s_waitcnt"]
    caught = 0
    for i in waits:
        name, a = prog.ops[i]
        n = int(a[0][len("lgkmcnt("):-1])
        prog.ops[i] = (name, [f"lgkmcnt({n + 1})"])
        try:
            for c in ((0, 1, 6, 3), (0, 3, 12, 3), (0, 0, 0, 3), (0, 0, 2, 1), (0, 1, 4, 1), (0, 0, 0, 1), (0, 1, 5, 2), (0, 0, 3, 2)):
                run_single(prog, words, cells[0][0], cells[0][1], table, c)
        except Hazard:
            caught += 1
        finally:
            prog.ops[i] = (name, a)
    # Over chunks 0 to 2 the eight controls reach far, straddling and near chunks with a chunk behind them and as the last
    # chunk.  The scan waits once per chunk on the line (before the kind test) and once per last chunk: 2 + 3 waits, and
    # each of them, raised by one, leaves the chunk's last read outstanding where it is used.
    assert len(waits) == 25 and caught >= 5, (len(waits), caught)
