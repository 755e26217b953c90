#!/usr/bin/env python3
"""Generates open-msspe-design_amd/csrc/row_bound_packed_pinned.inc: the predecessor scan of the PACKED bound instance
of thal_pairs_row.hip's 13-base kernel (k_pairs_bound_packed) as one inline-asm block over a slot table of ONE
register per slot, in a register map of its own (the whole kernel fits 128 VGPRs, four waves per SIMD):

    v76 .. v127   W[0 .. 51]   slot words  K << 17 | (cell value in coarse units + bias), bits 15 and 16 zero
    v74           the far accumulator   (chunks that lie entirely in rows i-2 and above)
    v75           the near accumulator  (the chunk that straddles rows i-2 / i-1 and the chunks of row i-1)
    everything else: the compiler's

The cell's minuend C keeps 0x7fff in its low 15 bits, so t = C - W never borrows into K: t >> 15 is the table address
as in the other instances, and the low 16 bits of t are  u = 0x7fff - bias - value  of the predecessor.  The table
holds  Tn = OFF - entry  (0: not available), so that  u + Tn = const - (entry + value): the candidate, negated and
shifted, and the running MAXIMUM of it is the minimum over the candidates.  A visit is

    v_sub_u32, v_lshrrev_b32, [ds_read_b32], v_mad_u32_u16 (u * 1 + Tn), half a v_max3_i32

The cell-side term Y of the far chunks is the same for every far entry of a cell: the caller adds it once to the far
minimum.  The straddling chunk subtracts it per slot (a wave-uniform mask), the chunks of row i-1 leave it out.
Every chunk's table reads are issued before the chunk in front of it is reduced (far, straddling and near alike), and
the waits are counted: s_waitcnt lgkmcnt(reads of the newer chunk).  The code is laid out so that a far chunk with
another chunk behind it -- nearly every chunk of a scan -- runs in a straight line: two tests, no branch taken.  With
the kinds dispatched by taken branches at every chunk the same kernel ran 9 % slower.
usage: tools/gen_row_bound_packed_asm.py > open-msspe-design_amd/csrc/row_bound_packed_pinned.inc

--ring: the scan k_pairs_bound_window runs (row_bound_ring_pinned.inc, macros MSSPE_BRG13_*).  With a window of two rows
only rows i-2 and i-1 are ever read again, so the windowed instance keeps its rows in a RING of three banks of 16
registers instead of the linear table (everything above the window is the kernel's one far candidate: thal_pairs_row.hip
run_pair_window):

    v76 .. v91, v92 .. v107, v108 .. v123   bank 0, 1, 2: row i lives in bank i % 3, its c-th cell in v(76 + 16 (i % 3) + c)
    v74, v75                                 the far and the near accumulator, as above

The slot word, the minuend, the table and the visit are unchanged.  A cell of row i visits bank (i-2) % 3 slots
0 .. %[WF]-1 into the far accumulator (the caller adds the cell-side term once) and bank (i-1) % 3 slots 0 .. %[WN]-1 into
the near one, and nothing else: no chunk straddles two rows (no per-slot mask, no %[Y]), none reaches above the window
(no %[START], no entry tree), and a register beyond a row's width -- it may hold a word of row i-3 -- is never read.
%[WF], %[WN] are the rows' widths (scalars, 0: no such row), %[WMAX] their maximum.
A row's first chunk is min(width, 4) slots.  The three rotations times the 5 x 5 sizes of the two first chunks are 75
straight-line leaves, entered through one tree of scalar compares on
    %[IDX] = ((i % 3) * 5 + min(WF, 4)) * 5 + min(WN, 4):
the far unit and the near unit are issued back to back, the far one is reduced under s_waitcnt lgkmcnt(near unit's
reads), the near one under lgkmcnt(0).  Rows are 3.2 wide on average, so this is the whole scan of two cells in three;
a leaf with a full chunk tests %[WMAX] > 4 and goes on to the rotation's wide path: for the slots 4.., 8.., 12 of either
row a test, a body per tail size (1 to 4 slots), issue, wait, reduce.
The two ring files keep their repeated parts as preprocessor macros -- I<n> (issue a unit of n slots), R<n> (reduce it),
LEAF_<sf>_<sn> (a leaf, by the two bank's registers), WIDE_<n> (a chunk of the wide path) -- so a leaf is one line; the
compiler sees the same flat instruction list (tests/test_pair_bound_ring_model.py expands them with the preprocessor).
usage: tools/gen_row_bound_packed_asm.py --ring > open-msspe-design_amd/csrc/row_bound_ring_pinned.inc

--ring --pair: two cells of one row in one pass (row_bound_ring_pair_pinned.inc, macros MSSPE_BRP13_*; operands %[CA]
%[CB], cell B accumulates into %[bf] / %[bn]).  The controls are the row's, so the tree is walked once for both.  A
leaf's units run far(A), near(A), far(B), near(B) through the two register sets in turn: a unit is reduced while the
one behind it is in flight (counted wait), and the unit two places on is issued into the registers it leaves.  The wide
path runs a chunk for both cells at once: one dispatch, B's reads in flight while A is reduced (cell A's wide path
followed by cell B's measured 1.7 ms per step slower: DESIGN 4.0).  A row of odd width ends on the single-cell scan.
usage: tools/gen_row_bound_packed_asm.py --ring --pair > open-msspe-design_amd/csrc/row_bound_ring_pair_pinned.inc
"""
import sys

FORMS = {(): (False, False), ("--ring",): (True, False), ("--ring", "--pair"): (True, True)}
if tuple(sys.argv[1:]) not in FORMS:
    sys.exit(__doc__)
RING, RING_PAIR = FORMS[tuple(sys.argv[1:])]
PFX = "MSSPE_BPK13"
KC = 4   # slots per chunk (6 and 8 measured slower: DESIGN 4.0)
NS, W0, ACCF, ACCN = 52, 76, 74, 75
TUPLES = [(76, 32), (108, 16), (124, 4)]
SIZES = [KC] * (NS // KC) + ([NS % KC] if NS % KC else [])
START = [sum(SIZES[:pc]) for pc in range(len(SIZES))]


def scan_asm():
    L = []
    a = lambda s: L.append(s)
    # operands: %[C] %[Y] v; %[NFAR] %[NRUN] %[NEAR] s; outputs v74, v75 (fixed);
    # temps, two sets of chunks in flight: %[a0..] / %[t0..] v hold t = C - W, then the candidate; %[v0..] v (2 KC) the
    # table address, then the loaded entry; %[yt] v;
    # immediate %[TOFF]
    nch = len(SIZES)
    SETS = ([f"%[a{e}]" for e in range(KC)], [f"%[t{e}]" for e in range(KC)])
    W = lambda pc, e: W0 + START[pc] + e

    def chunk_issue(pc):
        # t = C - W stays in regs[e] (its low 16 bits are the candidate's u); the address goes to the loaded value's
        # register, which the read overwrites
        t, n = SETS[pc & 1], SIZES[pc]
        v = [f"%[v{(pc & 1) * KC + e}]" for e in range(n)]
        for e in range(n):
            a(f"v_sub_u32 {t[e]}, %[C], v{W(pc, e)}")
        for e in range(n):
            a(f"v_lshrrev_b32 {v[e]}, 15, {t[e]}")
        for e in range(n):
            a(f"ds_read_b32 {v[e]}, {v[e]} offset:%c[TOFF]")

    def reduce(acc, regs, n):
        for e in range(0, n - 1, 2):
            a(f"v_max3_i32 v{acc}, v{acc}, {regs[e]}, {regs[e + 1]}")
        if n & 1:
            a(f"v_max_i32 v{acc}, v{acc}, {regs[n - 1]}")

    def process(pc, kind):
        t, n = SETS[pc & 1], SIZES[pc]
        v = [f"%[v{(pc & 1) * KC + e}]" for e in range(n)]
        for e in range(n):
            a(f"v_mad_u32_u16 {t[e]}, {t[e]}, 1, {v[e]}")
        if kind == "straddle":
            for e in range(n):
                a(f"s_cmp_gt_i32 %[NEAR], {START[pc] + e}")
                a("s_cselect_b64 vcc, -1, 0")
                a("v_cndmask_b32_e32 %[yt], 0, %[Y], vcc")
                a(f"v_sub_u32 {t[e]}, {t[e]}, %[yt]")
        reduce(ACCF if kind == "far" else ACCN, t, n)

    def dispatch(pc, tag, then):
        # this chunk by its kind: far (rows i-2 and above), straddling, or row i-1 alone; `then`: where to go on
        a(f"s_cmp_gt_i32 %[NFAR], {pc}")
        a(f"s_cbranch_scc0 L{tag}s{pc}_%=")
        process(pc, "far")
        a(f"s_branch {then}")
        a(f"L{tag}s{pc}_%=:")
        near_only(pc, tag, then)

    def near_only(pc, tag, then):
        a(f"s_cmp_gt_i32 %[NEAR], {START[pc]}")
        a(f"s_cbranch_scc0 L{tag}n{pc}_%=")
        process(pc, "straddle")
        a(f"s_branch {then}")
        a(f"L{tag}n{pc}_%=:")
        process(pc, "near")
        a(f"s_branch {then}")

    a(f"v_mov_b32 v{ACCF}, 0")
    a(f"v_mov_b32 v{ACCN}, 0")
    a("s_cmp_gt_i32 %[NRUN], 0")
    a("s_cbranch_scc0 Ldone%=")
    chunk_issue(0)
    # ---- the straight line: a far chunk with another chunk behind it.  The next chunk's reads are issued first, the
    #      wait is for this chunk's alone, and no branch is taken
    for pc in range(nch - 1):
        a(f"Lc{pc}_%=:")
        a(f"s_cmp_gt_i32 %[NRUN], {pc + 1}")
        a(f"s_cbranch_scc0 Lx{pc}_%=")
        chunk_issue(pc + 1)
        a(f"s_waitcnt lgkmcnt({SIZES[pc + 1]})")
        a(f"s_cmp_gt_i32 %[NFAR], {pc}")
        a(f"s_cbranch_scc0 Ly{pc}_%=")
        process(pc, "far")
    a(f"Lc{nch - 1}_%=:")
    a(f"Lx{nch - 1}_%=:")
    a("s_waitcnt lgkmcnt(0)")
    dispatch(nch - 1, "x", "Ldone%=")
    # ---- off the line: a straddling or near chunk with another behind it (its reads are in flight already) ...
    for pc in range(nch - 1):
        a(f"Ly{pc}_%=:")
        near_only(pc, "y", f"Lc{pc + 1}_%=")
    # ---- ... and the last chunk that runs, of whatever kind
    for pc in range(nch - 1):
        a(f"Lx{pc}_%=:")
        a("s_waitcnt lgkmcnt(0)")
        dispatch(pc, "x", "Ldone%=")
    a("Ldone%=:")
    return L


RING_BANKS, RING_BANK_REGS, RING_MAXW = 3, 16, 13


def ring_scan(pair):
    """(items of the scan, macro definitions).  An item is an instruction or label (str) or a macro call (name, args);
    the .inc keeps the units and the leaves as preprocessor macros, so that the file stays small enough to read."""
    PFX = "MSSPE_BRP13" if pair else "MSSPE_BRG13"
    items, defs, defined = [], [], set()
    a = lambda s: items.append(s)
    # operands: %[C] (pair: %[CA] %[CB]) v; %[IDX] %[WF] %[WN] %[WMAX] s; outputs v74, v75 (pair: cell A's; cell B's are
    # %[bf] %[bn]); temps, two units in flight: set a = %[ta0..3] / %[va0..3], set b = %[tb0..3] / %[vb0..3]
    sizes = [0, 1, 2, 3, 4]     # what a row leaves for a chunk: nothing, a tail, a full chunk
    nsz = len(sizes)
    CELLS = [("CA", {"far": f"v{ACCF}", "near": f"v{ACCN}"}), ("CB", {"far": "%[bf]", "near": "%[bn]"})] if pair \
        else [("C", {"far": f"v{ACCF}", "near": f"v{ACCN}"})]
    bank = lambda rot, role: W0 + RING_BANK_REGS * ((rot + (1 if role == "far" else 2)) % RING_BANKS)
    label = [0]
    P = lambda x: '" #' + x + ' "'      # a macro parameter, stringified into the instruction text

    def new_label(tag):
        label[0] += 1
        return f"L{tag}{label[0]}_%="

    def define(name, params, body):
        if name not in defined:
            defined.add(name)
            defs.append((name, params, body))

    def issue_text(st, C, regs):
        n = len(regs)
        return [f"v_sub_u32 %[t{st}{e}], %[{C}], v{regs[e]}" for e in range(n)] + \
               [f"v_lshrrev_b32 %[v{st}{e}], 15, %[t{st}{e}]" for e in range(n)] + \
               [f"ds_read_b32 %[v{st}{e}], %[v{st}{e}] offset:%c[TOFF]" for e in range(n)]

    def reduce_text(st, acc, n):
        return [f"v_mad_u32_u16 %[t{st}{e}], %[t{st}{e}], 1, %[v{st}{e}]" for e in range(n)] + \
               [f"v_max3_i32 {acc}, {acc}, %[t{st}{e}], %[t{st}{e + 1}]" for e in range(0, n - 1, 2)] + \
               ([f"v_max_i32 {acc}, {acc}, %[t{st}{n - 1}]"] if n & 1 else [])

    def issue(out, st, C, regs):
        # I<n>(set, minuend, the slots' registers)
        n = len(regs)
        define(f"I{n}", ["s", "C"] + [f"r{e}" for e in range(n)], issue_text(P("s"), P("C"), [P(f"r{e}") for e in range(n)]))
        out.append((f"I{n}", [st, C] + [str(r) for r in regs]))

    def reduce(out, st, acc, n):
        # R<n>(set, accumulator)
        define(f"R{n}", ["s", "acc"], reduce_text(P("s"), P("acc"), n))
        out.append((f"R{n}", [st, acc]))

    def wait(out, n):
        out.append(f"s_waitcnt lgkmcnt({n})")

    def leaf_body(out, far, near):
        # the rows' first chunks, both known: a straight line.  The units run far(A), near(A), far(B), near(B) through the
        # sets a, b in turn; a unit is reduced while the one behind it is in flight (its size is the wait's count), and
        # the unit two places on is issued into the registers the reduced one leaves
        regs = {"far": far, "near": near}
        units = [(c, role) for c in range(len(CELLS)) for role in ("far", "near") if regs[role]]
        for u, (c, role) in enumerate(units[:2]):
            issue(out, "ab"[u], CELLS[c][0], regs[role])
        for u, (c, role) in enumerate(units):
            wait(out, len(regs[units[u + 1][1]]) if u + 1 < len(units) else 0)
            reduce(out, "ab"[u & 1], CELLS[c][1][role], len(regs[role]))
            if u + 2 < len(units):
                c2, role2 = units[u + 2]
                issue(out, "ab"[u & 1], CELLS[c2][0], regs[role2])

    def leaf(rot, sf, sn):
        # LEAF_<sf>_<sn>(far row's registers, near row's registers)
        if sf or sn:
            params = [f"f{e}" for e in range(sf)] + [f"n{e}" for e in range(sn)]
            body = []
            leaf_body(body, [f"F{e}" for e in range(sf)], [f"N{e}" for e in range(sn)])
            sym = {f"F{e}": f"f{e}" for e in range(sf)}
            sym.update({f"N{e}": f"n{e}" for e in range(sn)})
            define(f"LEAF_{sf}_{sn}", params, [x if isinstance(x, str) else (x[0], [sym.get(y, y) for y in x[1]]) for x in body])
            a((f"LEAF_{sf}_{sn}", [str(bank(rot, "far") + e) for e in range(sf)] + [str(bank(rot, "near") + e) for e in range(sn)]))
        if KC in (sf, sn):
            a(f"s_cmp_gt_i32 %[WMAX], {KC}")
            a("s_cbranch_scc0 Ldone%=")
            a(f"s_branch Lwide{rot}_%=")
        else:
            a("s_branch Ldone%=")

    def by_size(W, base, cands, body):
        # W - base >= cands[0]: the largest of cands that fits runs
        if len(cands) == 1:
            body(cands[0])
            return
        mid = len(cands) // 2
        hi, end = new_label("h"), new_label("e")
        a(f"s_cmp_lt_i32 {W}, {base + cands[mid]}")
        a(f"s_cbranch_scc0 {hi}")
        by_size(W, base, cands[:mid], body)
        a(f"s_branch {end}")
        a(f"{hi}:")
        by_size(W, base, cands[mid:], body)
        a(f"{end}:")

    def wide(rot):
        # a row wider than one chunk (one row in five): its further chunks one at a time, each with a body per tail size.
        # The two-cell scan runs a chunk for both cells at once: one dispatch, B's reads in flight while A is reduced
        a(f"Lwide{rot}_%=:")
        for base in range(KC, RING_MAXW, KC):
            cands = [s for s in sizes if s and base + s <= RING_MAXW]
            for role, W in (("far", "%[WF]"), ("near", "%[WN]")):
                skip = new_label("s")
                a(f"s_cmp_gt_i32 {W}, {base}")
                a(f"s_cbranch_scc0 {skip}")

                def body(n, role=role, base=base):
                    # WIDE_<n>(accumulator of A [, of B], the slots' registers)
                    accs = [f"acc{c}" for c in range(len(CELLS))]
                    out = []
                    for st, (C, _) in enumerate(CELLS):
                        issue(out, "ab"[st], C, [f"r{e}" for e in range(n)])
                    for st in range(len(CELLS)):
                        wait(out, n if st + 1 < len(CELLS) else 0)
                        reduce(out, "ab"[st], accs[st], n)
                    define(f"WIDE_{n}", accs + [f"r{e}" for e in range(n)], out)
                    a((f"WIDE_{n}", [acc[role] for _, acc in CELLS] + [str(bank(rot, role) + base + e) for e in range(n)]))

                by_size(W, base, cands, body)
                a(f"{skip}:")
            if base + KC < RING_MAXW:
                a(f"s_cmp_gt_i32 %[WMAX], {base + KC}")
                a("s_cbranch_scc0 Ldone%=")
        a("s_branch Ldone%=")

    def enter(lo, hi):
        # %[IDX] = (rotation * nsz + far size's index) * nsz + near size's index
        if lo == hi:
            rot, fi, ni = lo // (nsz * nsz), lo // nsz % nsz, lo % nsz
            leaf(rot, sizes[fi], sizes[ni])
            return
        mid = (lo + hi + 1) // 2
        a(f"s_cmp_lt_i32 %[IDX], {mid}")
        a(f"s_cbranch_scc0 Le{mid}_{hi}_%=")
        enter(lo, mid - 1)
        a(f"Le{mid}_{hi}_%=:")
        enter(mid, hi)

    for _, acc in CELLS:
        a(f"v_mov_b32 {acc['far']}, 0")
        a(f"v_mov_b32 {acc['near']}, 0")
    enter(0, RING_BANKS * nsz * nsz - 1)
    for rot in range(RING_BANKS):
        wide(rot)
    a("Ldone%=:")
    return PFX, items, defs, nsz


def ring_render(PFX, items, defs):
    """The macro definitions and the *_SCAN_ASM macro as text.  An instruction is one string literal; a compare and the
    branch on it share a line."""
    lit = lambda s: '"' + s + '\\n\\t"'
    call = lambda x: f"{PFX}_{x[0]}({', '.join(x[1])})"
    piece = lambda x: lit(x) if isinstance(x, str) else call(x)

    def lines_of(seq):
        out = []
        for x in seq:
            if isinstance(x, str) and x.startswith("s_cbranch") and out and out[-1].startswith('"s_cmp'):
                out[-1] += " " + lit(x)
            else:
                out.append(piece(x))
        return out

    text = []
    for name, params, body in defs:
        text.append(f"#define {PFX}_{name}({', '.join(params)}) \\")
        if all(isinstance(x, str) for x in body):
            text.append(" \\\n".join("    " + lit(x) for x in body))
        else:
            text.append("    " + " ".join(piece(x) for x in body))
    text.append(f"#define {PFX}_SCAN_ASM \\")
    text.append(" \\\n".join("    " + l for l in lines_of(items)))
    return "\n".join(text)


if RING:
    PFX, items, defs, nsz = ring_scan(RING_PAIR)
    print(f"// GENERATED by tools/gen_row_bound_packed_asm.py --ring{' --pair' if RING_PAIR else ''}"
          " -- do not edit (see that file for the why and the register map)")
    print(f"#define {PFX}_KC {KC}")
    print(f"#define {PFX}_W0 {W0}")
    print(f"#define {PFX}_BANK {RING_BANK_REGS}")
    print(f"#define {PFX}_GRAN 1")   # read by nothing in this tree: 84f3bf2's tests/test_pair_bound_ring_model.py reads it on import
    print(f"#define {PFX}_NSZ {nsz}")
    print(ring_render(PFX, items, defs))
    print(f'#define {PFX}_SCAN_CLOBBERS "scc", "memory"')
    temps = [f"{k}{s}{e}" for k in "tv" for s in "ab" for e in range(KC)]
    print(f"#define {PFX}_TEMP_NAMES " + ", ".join(temps))
    print(f"#define {PFX}_TEMPS_OUT " + ", ".join(f'[{t}] "=&v"({t})' for t in temps))
    if RING_PAIR:
        print(f'#define {PFX}_ACC_OUT(far_a, near_a, far_b, near_b) "=&{{v{ACCF}}}"(far_a), "=&{{v{ACCN}}}"(near_a), '
              '[bf] "=&v"(far_b), [bn] "=&v"(near_b)')
    else:
        print(f'#define {PFX}_ACC_OUT(far, near) "=&{{v{ACCF}}}"(far), "=&{{v{ACCN}}}"(near)')
    names = ["Ra", "Rb", "Rc"]
    banks = [(W0 + RING_BANK_REGS * b, RING_BANK_REGS) for b in range(RING_BANKS)]
    print(f"#define {PFX}_TUPLES_IN(" + ", ".join(names) + ") " +
          ", ".join('"{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(banks, names)))
    print(f"#define {PFX}_TUPLES_INOUT(" + ", ".join(names) + ") " +
          ", ".join('"+{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(banks, names)))
    sys.exit(0)

print("// GENERATED by tools/gen_row_bound_packed_asm.py -- do not edit (see that file for the why and the register map)")
print(f"#define {PFX}_KC {KC}")
print(f"#define {PFX}_W0 {W0}")
print(f"#define {PFX}_SCAN_ASM \\")
print(" \\\n".join('    "' + l + '\\n\\t"' for l in scan_asm()))
print(f'#define {PFX}_SCAN_CLOBBERS "vcc", "scc", "memory"')
temps = [f"a{e}" for e in range(KC)] + [f"t{e}" for e in range(KC)] + [f"v{e}" for e in range(2 * KC)] + ["yt"]
print(f"#define {PFX}_TEMP_NAMES " + ", ".join(temps))
print(f"#define {PFX}_TEMPS_OUT " + ", ".join(f'[{t}] "=&v"({t})' for t in temps))
print(f'#define {PFX}_ACC_OUT(far, near) "=&{{v{ACCF}}}"(far), "=&{{v{ACCN}}}"(near)')
names = ["Wa", "Wb", "Wc"]
print(f"#define {PFX}_TUPLES_IN(" + ", ".join(names) + ") " +
      ", ".join('"{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(TUPLES, names)))
print(f"#define {PFX}_TUPLES_INOUT(" + ", ".join(names) + ") " +
      ", ".join('"+{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(TUPLES, names)))
