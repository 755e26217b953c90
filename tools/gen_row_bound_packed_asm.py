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

--window F: the WINDOWED instance's scan (k_pairs_bound_window; row_bound_window_pinned.inc, macros MSSPE_BWN13_*).  The
same chunks, kinds and waits, but the scan of a cell in row i ENTERS the unrolled sequence at the chunk %[START] that
holds the first slot of row i - F (a scalar: a wave holds one composition) instead of at chunk 0: a tree of scalar
compares leads to that chunk's issue, which joins the straight line.  Everything above the window is the kernel's one
far candidate (thal_pairs_row.hip run_pair_packed); F itself only reaches the kernel, as MSSPE_BWN13_F.
usage: tools/gen_row_bound_packed_asm.py --window 2 > open-msspe-design_amd/csrc/row_bound_window_pinned.inc

--window F --pair: the windowed scan of TWO cells of one row in one pass (row_bound_window_pair_pinned.inc, macros
MSSPE_BWP13_*).  Two cells of a row never depend on each other (a predecessor lies strictly above and left of its cell),
and %[START], %[NRUN], %[NFAR], %[NEAR] are the row's, so the NRUN > START test, the entry tree and every chunk's
has-next and kind tests run once for both.  Operands %[CA] %[YA] %[CB] %[YB]; cell A accumulates into v74 / v75, cell B
into %[bf] / %[bn] (the compiler's).  The two register sets that hold two chunks of one cell above hold the SAME chunk
of the two cells here, and the units alternate A(pc), B(pc), A(pc+1), B(pc+1), ...: a chunk with another behind it is
    wait for A(pc) (counted: B(pc)'s reads stay in flight), reduce A(pc), issue A(pc+1),
    wait for B(pc) (counted: A(pc+1)'s stay in flight),      reduce B(pc), issue B(pc+1)
and the last chunk waits for zero before B.  The straddling chunk's per-slot mask is formed per cell.
usage: tools/gen_row_bound_packed_asm.py --window 2 --pair > open-msspe-design_amd/csrc/row_bound_window_pair_pinned.inc
"""
import sys

PAIR = len(sys.argv) == 4 and sys.argv[3] == "--pair"
WINDOW = int(sys.argv[2]) if len(sys.argv) == 3 + PAIR and sys.argv[1] == "--window" else 0
if (len(sys.argv) != 1 and not WINDOW) or WINDOW not in (0, 2, 3) or (PAIR and WINDOW != 2):
    sys.exit(__doc__)
PFX = "MSSPE_BWP13" if PAIR else "MSSPE_BWN13" if WINDOW else "MSSPE_BPK13"
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
    if WINDOW:
        # the entry: chunk %[START] .. %[NRUN] - 1 run (none: START >= NRUN); a leaf issues its chunk and joins the line
        def enter(lo, hi):
            if lo == hi:
                chunk_issue(lo)
                a(f"s_branch Lc{lo}_%=")
                return
            mid = (lo + hi + 1) // 2
            a(f"s_cmp_lt_i32 %[START], {mid}")
            a(f"s_cbranch_scc0 Le{mid}_{hi}_%=")
            enter(lo, mid - 1)
            a(f"Le{mid}_{hi}_%=:")
            enter(mid, hi)

        a("s_cmp_gt_i32 %[NRUN], %[START]")
        a("s_cbranch_scc0 Ldone%=")
        enter(0, nch - 1)
    else:
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


def pair_scan_asm():
    L = []
    a = lambda s: L.append(s)
    # operands: %[CA] %[YA] %[CB] %[YB] v; %[NFAR] %[NRUN] %[NEAR] %[START] s; outputs v74, v75 (cell A, fixed),
    # %[bf] %[bn] v (cell B); temps: cell A's chunk in %[a0..] / %[v0..], cell B's in %[t0..] / %[v4..]; %[yt] v
    nch = len(SIZES)
    CELLS = {"A": ("%[CA]", "%[YA]", [f"%[a{e}]" for e in range(KC)], [f"%[v{e}]" for e in range(KC)], f"v{ACCF}", f"v{ACCN}"),
             "B": ("%[CB]", "%[YB]", [f"%[t{e}]" for e in range(KC)], [f"%[v{KC + e}]" for e in range(KC)], "%[bf]", "%[bn]")}

    def issue(cell, pc):
        C, _, t, v, _, _ = CELLS[cell]
        n = SIZES[pc]
        for e in range(n):
            a(f"v_sub_u32 {t[e]}, {C}, v{W0 + START[pc] + e}")
        for e in range(n):
            a(f"v_lshrrev_b32 {v[e]}, 15, {t[e]}")
        for e in range(n):
            a(f"ds_read_b32 {v[e]}, {v[e]} offset:%c[TOFF]")

    def process(cell, pc, kind):
        _, Y, t, v, far, near = CELLS[cell]
        n = SIZES[pc]
        for e in range(n):
            a(f"v_mad_u32_u16 {t[e]}, {t[e]}, 1, {v[e]}")
        if kind == "straddle":
            for e in range(n):
                a(f"s_cmp_gt_i32 %[NEAR], {START[pc] + e}")
                a("s_cselect_b64 vcc, -1, 0")
                a(f"v_cndmask_b32_e32 %[yt], 0, {Y}, vcc")
                a(f"v_sub_u32 {t[e]}, {t[e]}, %[yt]")
        acc = far if kind == "far" else near
        for e in range(0, n - 1, 2):
            a(f"v_max3_i32 {acc}, {acc}, {t[e]}, {t[e + 1]}")
        if n & 1:
            a(f"v_max_i32 {acc}, {acc}, {t[n - 1]}")

    def body(pc, kind, nxt):
        # in flight on entry: A(pc), B(pc), in that order
        a(f"s_waitcnt lgkmcnt({SIZES[pc]})")
        process("A", pc, kind)
        if nxt:
            issue("A", pc + 1)
        a(f"s_waitcnt lgkmcnt({SIZES[pc + 1] if nxt else 0})")
        process("B", pc, kind)
        if nxt:
            issue("B", pc + 1)

    def dispatch(pc, tag, nxt, then):
        a(f"s_cmp_gt_i32 %[NFAR], {pc}")
        a(f"s_cbranch_scc0 L{tag}s{pc}_%=")
        body(pc, "far", nxt)
        a(f"s_branch {then}")
        a(f"L{tag}s{pc}_%=:")
        near_only(pc, tag, nxt, then)

    def near_only(pc, tag, nxt, then):
        a(f"s_cmp_gt_i32 %[NEAR], {START[pc]}")
        a(f"s_cbranch_scc0 L{tag}n{pc}_%=")
        body(pc, "straddle", nxt)
        a(f"s_branch {then}")
        a(f"L{tag}n{pc}_%=:")
        body(pc, "near", nxt)
        a(f"s_branch {then}")

    def enter(lo, hi):
        if lo == hi:
            issue("A", lo)
            issue("B", lo)
            a(f"s_branch Lc{lo}_%=")
            return
        mid = (lo + hi + 1) // 2
        a(f"s_cmp_lt_i32 %[START], {mid}")
        a(f"s_cbranch_scc0 Le{mid}_{hi}_%=")
        enter(lo, mid - 1)
        a(f"Le{mid}_{hi}_%=:")
        enter(mid, hi)

    for acc in (f"v{ACCF}", f"v{ACCN}", "%[bf]", "%[bn]"):
        a(f"v_mov_b32 {acc}, 0")
    a("s_cmp_gt_i32 %[NRUN], %[START]")
    a("s_cbranch_scc0 Ldone%=")
    enter(0, nch - 1)
    # ---- the straight line: a far chunk with another chunk behind it, both cells, no branch taken
    for pc in range(nch - 1):
        a(f"Lc{pc}_%=:")
        a(f"s_cmp_gt_i32 %[NRUN], {pc + 1}")
        a(f"s_cbranch_scc0 Lx{pc}_%=")
        a(f"s_cmp_gt_i32 %[NFAR], {pc}")
        a(f"s_cbranch_scc0 Ly{pc}_%=")
        body(pc, "far", True)
    a(f"Lc{nch - 1}_%=:")
    a(f"Lx{nch - 1}_%=:")
    dispatch(nch - 1, "x", False, "Ldone%=")
    # ---- off the line: a straddling or near chunk with another behind it ...
    for pc in range(nch - 1):
        a(f"Ly{pc}_%=:")
        near_only(pc, "y", True, f"Lc{pc + 1}_%=")
    # ---- ... and the last chunk that runs, of whatever kind
    for pc in range(nch - 1):
        a(f"Lx{pc}_%=:")
        dispatch(pc, "x", False, "Ldone%=")
    a("Ldone%=:")
    return L


print(f"// GENERATED by tools/gen_row_bound_packed_asm.py{f' --window {WINDOW}' if WINDOW else ''}{' --pair' if PAIR else ''} -- do not edit (see that file for the why and the register map)")
if WINDOW:
    print(f"#define {PFX}_F {WINDOW}")
print(f"#define {PFX}_KC {KC}")
print(f"#define {PFX}_W0 {W0}")
print(f"#define {PFX}_SCAN_ASM \\")
print(" \\\n".join('    "' + l + '\\n\\t"' for l in (pair_scan_asm() if PAIR else scan_asm())))
print(f'#define {PFX}_SCAN_CLOBBERS "vcc", "scc", "memory"')
temps = [f"a{e}" for e in range(KC)] + [f"t{e}" for e in range(KC)] + [f"v{e}" for e in range(2 * KC)] + ["yt"]
print(f"#define {PFX}_TEMP_NAMES " + ", ".join(temps))
print(f"#define {PFX}_TEMPS_OUT " + ", ".join(f'[{t}] "=&v"({t})' for t in temps))
if PAIR:
    print(f'#define {PFX}_ACC_OUT(far_a, near_a, far_b, near_b) "=&{{v{ACCF}}}"(far_a), "=&{{v{ACCN}}}"(near_a), '
          '[bf] "=&v"(far_b), [bn] "=&v"(near_b)')
else:
    print(f'#define {PFX}_ACC_OUT(far, near) "=&{{v{ACCF}}}"(far), "=&{{v{ACCN}}}"(near)')
names = ["Wa", "Wb", "Wc"]
print(f"#define {PFX}_TUPLES_IN(" + ", ".join(names) + ") " +
      ", ".join('"{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(TUPLES, names)))
print(f"#define {PFX}_TUPLES_INOUT(" + ", ".join(names) + ") " +
      ", ".join('"+{v[%d:%d]}"(%s)' % (r0, r0 + ln - 1, nm) for (r0, ln), nm in zip(TUPLES, names)))
