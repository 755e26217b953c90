"""The ring scans of k_pairs_bound_window run in an interpreter, without a GPU (tools/gen_row_bound_packed_asm.py --ring
and --ring --pair; tests/scan_interpreter.py).

The windowed instance keeps the last three rows in three banks of 16 registers (row i in bank i % 3, its c-th cell in
register 76 + 16 * (i % 3) + c) and a cell of row i visits bank (i-2) % 3 slots 0 .. wf-1 into the far accumulator and
bank (i-1) % 3 slots 0 .. wn-1 into the near one: nothing else.  For every (rotation, wf, wn) in 3 x 0..13 x 0..13,
with random slot words and a random table (a third of its entries "not available"), every register the scan must not
visit -- the third bank, and a bank's registers from its row's width upwards -- holds a word whose candidate would win
if it were read:
the accumulators == the direct formula over exactly the window's slots, the two-cell scan == the single scan per
cell, no Hazard, no read outstanding at the end.

The visit count: over seeded random 13-mer pairs the ring visits w(i-2) + w(i-1) slots per cell; a linear table's
chunk-aligned count is printed beside it."""
import os
import random
import re
import subprocess

import pytest

from scan_interpreter import ROOT, Hazard, Program, generated, s32

CSRC = ROOT / "open-msspe-design_amd" / "csrc"
SINGLE_INC, PAIR_INC = CSRC / "row_bound_ring_pinned.inc", CSRC / "row_bound_ring_pair_pinned.inc"
KC, W0, BANK, MAXW = 4, 76, 16, 13
OFF = 1 << 28
POISON_WINS = OFF + 200000           # above every candidate a visited slot can give (OFF + 40000 + 0x7fff)


def macro(text, name):
    return int(re.search(rf"#define \w+_{name} (\d+)\n", text).group(1))


def scan_lines(path, pfx):
    """The instructions and labels of <pfx>_SCAN_ASM as the compiler sees them.  The ring .inc files keep their units and
    leaves as preprocessor macros (scan_interpreter.scan_lines reads flat files only), so the C preprocessor expands the
    committed file and the adjacent string literals are joined."""
    src = f'#include "{path}"\n{pfx}_SCAN_ASM\n'
    out = subprocess.run([os.environ.get("CXX", "g++"), "-E", "-P", "-x", "c++", "-"], input=src, capture_output=True, text=True,
                         check=True).stdout
    assert pfx not in out, "a macro of the .inc is left unexpanded"
    text = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', out))
    assert re.sub(r'"(?:[^"\\]|\\.)*"|\s', "", out) == "", "something beside string literals"
    lines = text.split("\\n\\t")
    assert lines[-1] == "" and len(lines) > 1000
    return lines[:-1]


@pytest.fixture(scope="module")
def single():
    return Program(scan_lines(SINGLE_INC, "MSSPE_BRG13"))


@pytest.fixture(scope="module")
def pair():
    return Program(scan_lines(PAIR_INC, "MSSPE_BRP13"))


def test_committed_ring_scans_are_the_generators_output():
    for path, args, pfx in ((SINGLE_INC, ("--ring",), "MSSPE_BRG13"), (PAIR_INC, ("--ring", "--pair"), "MSSPE_BRP13")):
        text = generated(*args)
        assert text == path.read_text(), path.name
        assert macro(text, "W0") == W0 and macro(text, "BANK") == BANK
        assert pfx in text and not any(p in text for p in {"MSSPE_BRG13", "MSSPE_BRP13", "MSSPE_BPK13"} - {pfx})
        assert "START" not in text and "%[Y" not in text      # no entry chunk, no straddling kind


def make_case(rng, rot, wf, wn):
    """Registers of the three banks, two cells' minuends and a table.  Real slot words have an even K below 900 and the
    minuends an even K above it, so a real visit reads an even table word (address / 4); the words of registers that must
    not be visited have an odd K, and the table answers an odd word with a candidate that wins."""
    fb, nb = (rot + 1) % 3, (rot + 2) % 3
    regs = {}
    for b in range(3):
        w = wf if b == fb else wn if b == nb else 0
        for c in range(BANK):
            if c < w:
                word = (2 * rng.randrange(0, 450) << 17) | rng.randrange(0, 0x8000)
            else:
                word = ((2 * rng.randrange(0, 450) + 1) << 17) | rng.randrange(0, 0x8000)
            regs[f"v{W0 + BANK * b + c}"] = word
    cells = [(2 * rng.randrange(500, 2000) << 17) | 0x7fff for _ in range(2)]
    seed = rng.randrange(1 << 30)

    def table(addr, area="TOFF"):
        assert area == "TOFF" and addr % 4 == 0, addr
        word = addr // 4
        if word & 1:
            return POISON_WINS
        x = random.Random(seed * 8191 + addr)
        return 0 if x.random() < 1 / 3 else OFF - x.randrange(-40000, 40000)

    return regs, cells, table


def formula(regs, C, table, rot, wf, wn):
    out = []
    for b, w in (((rot + 1) % 3, wf), ((rot + 2) % 3, wn)):
        acc = 0
        for c in range(w):
            t = (C - regs[f"v{W0 + BANK * b + c}"]) & 0xffffffff
            acc = max(acc, s32((t & 0xffff) + table(t >> 15)))
        out.append(acc & 0xffffffff)
    return tuple(out)


def controls(text, rot, wf, wn):
    nsz = macro(text, "NSZ")
    idx = (rot * nsz + min(wf, KC)) * nsz + min(wn, KC)
    return {"%[IDX]": idx, "%[WF]": wf, "%[WN]": wn, "%[WMAX]": max(wf, wn)}


SINGLE_TEXT, PAIR_TEXT = SINGLE_INC.read_text(), PAIR_INC.read_text()


def run_single(prog, regs, C, table, rot, wf, wn):
    v = dict(regs)
    v["%[C]"] = C
    out = prog.run(v, controls(SINGLE_TEXT, rot, wf, wn), table)
    assert all(out[r] == w for r, w in regs.items())      # the banks are read only
    return out["v74"], out["v75"]


def run_pair(prog, regs, cells, table, rot, wf, wn):
    v = dict(regs)
    v["%[CA]"], v["%[CB]"] = cells
    out = prog.run(v, controls(PAIR_TEXT, rot, wf, wn), table)
    assert all(out[r] == w for r, w in regs.items())
    return (out["v74"], out["v75"]), (out["%[bf]"], out["%[bn]"])


def all_windows():
    return [(rot, wf, wn) for rot in range(3) for wf in range(MAXW + 1) for wn in range(MAXW + 1)]


def test_table_geometry_of_the_case():
    """An address is (K of the minuend - K of the word) * 4 exactly: the field never borrows into K."""
    rng = random.Random(7000)
    regs, cells, _ = make_case(rng, 0, 13, 13)
    for w in regs.values():
        t = (cells[0] - w) & 0xffffffff
        assert (t >> 15) == ((cells[0] >> 17) - (w >> 17)) * 4 and (t & 0xffff) == 0x7fff - (w & 0x7fff)


def test_ring_scans_equal_the_formula_over_the_window_alone(single, pair):
    rng = random.Random(7100)
    real = 0
    for rot, wf, wn in all_windows():
        regs, cells, table = make_case(rng, rot, wf, wn)
        got = run_pair(pair, regs, cells, table, rot, wf, wn)
        for cell, C in zip(got, cells):
            want = formula(regs, C, table, rot, wf, wn)
            assert max(want) < POISON_WINS
            assert cell == want, ((rot, wf, wn), "formula")
            assert run_single(single, regs, C, table, rot, wf, wn) == want, ((rot, wf, wn), "single scan")
            real += want[0] > 0x10000 or want[1] > 0x10000
    assert real > 1000      # the accumulators hold real candidates, not stored zeros only


def test_a_visit_outside_the_window_would_be_seen(single):
    """The check has teeth: widen the near row by one register and the scan returns the candidate that must not win."""
    rng = random.Random(7200)
    for rot in range(3):
        regs, cells, table = make_case(rng, rot, 3, 2)
        ctl = controls(SINGLE_TEXT, rot, 3, 3)
        v = dict(regs)
        v["%[C]"] = cells[0]
        out = single.run(v, ctl, table)
        assert s32(out["v75"]) >= POISON_WINS and s32(out["v74"]) < POISON_WINS


def test_interpreter_finds_a_wrong_wait(single, pair):
    """Every wait the listed windows reach, made to count one read too many, raises Hazard."""
    rng = random.Random(7300)
    wins = [(0, 4, 4), (1, 3, 2), (2, 2, 0), (0, 0, 1), (1, 6, 9), (2, 13, 13)]
    cases = [(w, make_case(rng, *w)) for w in wins]
    for prog in (single, pair):
        reached = set()
        run = prog.run

        def trace(i):      # which waits the windows reach: run with each wait raised and see whether anything changes
            name, a = prog.ops[i]
            n = int(a[0][len("lgkmcnt("):-1])
            prog.ops[i] = (name, [f"lgkmcnt({n + 1})"])
            try:
                for w, (regs, cells, table) in cases:
                    if prog is pair:
                        run_pair(prog, regs, cells, table, *w)
                    else:
                        run_single(prog, regs, cells[0], table, *w)
            except Hazard:
                return True
            finally:
                prog.ops[i] = (name, a)
            return False

        waits = [i for i, (name, _) in enumerate(prog.ops) if name == "s_waitcnt"]
        caught = sum(trace(i) for i in waits)
        # six windows: each reaches at least one wait per unit of its first chunks (two units a cell where both rows hold
        # cells), and the wide ones further waits
        assert caught >= (10 if prog is pair else 8), caught


# ---- how many slots a cell visits -----------------------------------------------------------------------------------------
def widths_of(row, col):
    """Stored rows' widths and first slots, as row_starts of tests/test_gpu_pair_bound_window.py derives them: row i takes
    as many slots as col has bases complementary to row[i]; the last row is stored nowhere."""
    comp = {x: col.count(x) for x in "ACGT"}
    widths = [comp["TGCA"["ACGT".index(x)]] for x in row]
    starts, s = [], 0
    for w in widths[:-1]:
        starts.append(s)
        s += w
    return widths, starts, s


def test_visits_per_cell():
    rng = random.Random(20000)
    cells = ring = exact = linear = skipped = 0
    for _ in range(20000):
        row = "".join(rng.choice("ACGT") for _ in range(13))
        col = "".join(rng.choice("ACGT") for _ in range(13))
        widths, starts, total = widths_of(row, col)
        if total > 52:      # the sizing rule hands such a pair on unbounded
            skipped += 1
            continue
        starts = starts + [total]
        for i, w in enumerate(widths):
            wf = widths[i - 2] if i >= 2 else 0
            wn = widths[i - 1] if i >= 1 else 0
            s_far = starts[i - 2] if i >= 2 else 0
            s_row = starts[i] if i < 13 else total
            # the linear table: chunks start(i-2) / 4 up to ceil(start(i) / 4), four slots each
            lin = ((s_row + KC - 1) // KC - s_far // KC) * KC if s_row > s_far else 0
            assert lin >= wf + wn
            cells += w
            exact += w * (wf + wn)
            ring += w * (wf + wn)
            linear += w * lin
    print(f"{cells / (20000 - skipped):.1f} cells per pair; slots visited per cell: linear table {linear / cells:.2f}, "
          f"ring {ring / cells:.2f}, rows i-2 and i-1 alone {exact / cells:.2f}")
    assert ring == exact and exact <= ring <= linear
    assert 5.5 < exact / cells < 5.9 and 7.9 < linear / cells < 8.5
