"""The generated windowed scans run in an interpreter, without a GPU (tools/gen_row_bound_packed_asm.py --window 2 and
--window 2 --pair; tests/scan_interpreter.py).

The two-cell scan of k_pairs_bound_window (row_bound_window_pair_pinned.inc) walks the entry tree and every chunk's tests
once for two cells of a row and interleaves the two cells' table reads under counted waits.  A missing or miscounted
wait gives silently wrong minima on the device; here the interpreter delivers every LDS value at the last moment its
wait allows and raises when a register is used or overwritten while its read is outstanding.

For every reachable (START, NFAR, NEAR, NRUN) -- every (first slot of row i-2, of row i-1, of row i) with rows up to 13
wide in a table of up to 52 slots -- random slot words and a random table (a third of its entries "not available"):
the two-cell scan's four accumulators == the single-cell windowed scan's, run once per cell == the direct formula over
the visited slots."""
import random

import pytest

from scan_interpreter import ROOT, Hazard, Program, generated, s32, scan_lines

CSRC = ROOT / "open-msspe-design_amd" / "csrc"
KC, NS, W0, F = 4, 52, 76, 2
OFF = 1 << 28


@pytest.fixture(scope="module")
def single():
    return Program(scan_lines((CSRC / "row_bound_window_pinned.inc").read_text()))


@pytest.fixture(scope="module")
def pair():
    return Program(scan_lines((CSRC / "row_bound_window_pair_pinned.inc").read_text()))


def test_committed_pair_scan_is_the_generators_output():
    text = generated("--window", str(F), "--pair")
    assert text == (CSRC / "row_bound_window_pair_pinned.inc").read_text()
    assert f"#define MSSPE_BWP13_F {F}\n" in text and "MSSPE_BWN13" not in text and "MSSPE_BPK13" not in text


def controls():
    """Every distinct (START, NFAR, NEAR, NRUN) the kernel can pass: s2 <= s1 <= r the first slots of rows i-2, i-1, i."""
    seen = set()
    for s2 in range(NS + 1):
        for s1 in range(s2, min(s2 + 13, NS) + 1):
            for r in range(s1, min(s1 + 13, NS) + 1):
                seen.add((s2 // KC, s1 // KC, s1, (r + KC - 1) // KC))
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
    v = {f"v{W0 + s}": w for s, w in enumerate(words)}
    v.update({"%[C]": C, "%[Y]": Y & 0xffffffff})
    out = prog.run(v, {"%[START]": start, "%[NFAR]": nfar, "%[NEAR]": near, "%[NRUN]": nrun}, table)
    assert [out[f"v{W0 + s}"] for s in range(NS)] == words      # the slot table is read only
    return out["v74"], out["v75"]


def run_pair(prog, words, cells, table, ctl):
    start, nfar, near, nrun = ctl
    (CA, YA), (CB, YB) = cells
    v = {f"v{W0 + s}": w for s, w in enumerate(words)}
    v.update({"%[CA]": CA, "%[YA]": YA & 0xffffffff, "%[CB]": CB, "%[YB]": YB & 0xffffffff})
    out = prog.run(v, {"%[START]": start, "%[NFAR]": nfar, "%[NEAR]": near, "%[NRUN]": nrun}, table)
    assert [out[f"v{W0 + s}"] for s in range(NS)] == words
    return (out["v74"], out["v75"]), (out["%[bf]"], out["%[bn]"])


def test_single_scan_equals_the_formula_under_counted_waits(single):
    rng = random.Random(6100)
    ctls = controls()
    ran = 0
    for ctl in ctls:
        words, cells, table = make_case(rng)
        C, Y = cells[0]
        got = run_single(single, words, C, Y, table, ctl)
        assert got == formula(words, C, Y, table, *ctl), ctl
        ran += ctl[3] > ctl[0]
    assert ran > 500 and {c[0] for c in ctls} == set(range(NS // KC + 1))      # every entry chunk, and START = 13 (nothing runs)


def test_pair_scan_equals_two_single_scans_and_the_formula(single, pair):
    rng = random.Random(6200)
    kinds = set()
    for ctl in controls():
        words, cells, table = make_case(rng)
        got = run_pair(pair, words, cells, table, ctl)
        for cell, (C, Y) in zip(got, cells):
            want = formula(words, C, Y, table, *ctl)
            assert cell == want, (ctl, "formula")
            assert cell == run_single(single, words, C, Y, table, ctl), (ctl, "single scan")
        start, nfar, near, nrun = ctl
        for pc in range(start, nrun):
            kinds.add(("far" if nfar > pc else "straddle" if near > pc * KC else "near", pc + 1 < nrun, pc == start))
    # every chunk kind with and without a chunk behind it, as the entry chunk and behind it
    assert len(kinds) == 12


def test_interpreter_finds_a_wrong_wait(single, pair):
    """The check has teeth: every reached wait, made to count one read too many, raises Hazard (the interpreter delivers a
    value at the last moment its wait allows, so the chunk's last read is still outstanding where it is used)."""
    rng = random.Random(6300)
    words, cells, table = make_case(rng)
    ctl = (0, 1, 6, 3)      # a far, a straddling and a near chunk
    run_pair(pair, words, cells, table, ctl)
    for prog in (single, pair):
        waits = [i for i, (name, a) in enumerate(prog.ops) if name == "s_waitcnt"]
        caught = 0
        for i in waits:
            name, a = prog.ops[i]
            n = int(a[0][len("lgkmcnt("):-1])
            prog.ops[i] = (name, [f"lgkmcnt({n + 1})"])
            try:
                for c in ((0, 1, 6, 3), (0, 3, 12, 3), (0, 0, 0, 3), (0, 0, 2, 1), (0, 1, 4, 1), (0, 0, 0, 1), (0, 1, 5, 2), (0, 0, 3, 2)):
                    if prog is pair:
                        run_pair(prog, words, cells, table, c)
                    else:
                        run_single(prog, words, cells[0][0], cells[0][1], table, c)
            except Hazard:
                caught += 1
            finally:
                prog.ops[i] = (name, a)
        # Over chunks 0 to 2 the eight controls reach 13 bodies: far, straddling and near with a chunk behind them at chunk
        # 0, the same at chunk 1, and far, straddling and near as the last chunk at chunks 0, 1 and 2 less the two that no
        # control forms.  Each of their waits, raised by one, leaves the chunk's last read outstanding where it is used.
        # The single scan waits once per chunk on the line (before the kind test) and once per last chunk: 2 + 3 waits;
        # the two-cell scan waits twice per body.
        assert caught >= (26 if prog is pair else 5), caught
