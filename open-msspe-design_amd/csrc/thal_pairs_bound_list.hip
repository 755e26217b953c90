// thal_pairs_bound_list.hip -- the bound list stage: a lower bound of thal ANY's dG for the pairs of list U.
//
// The bound first stage (thal_pairs_row.hip k_pairs_bound) bounds the lanes that stay in their wave.  A lane that
// leaves it -- 53..63 stored cells, dragged, shed by the slot fit -- used to join the true survivors on list 0 and pay
// the exact list stages' price although nothing had tried to prove it harmless.  Such lanes go to list U instead, once
// per unordered pair under the mirror, and this kernel computes for each of them what k_pairs_bound computes for the
// others: the plain minimum over all chains  left end term, (stacked pair | loop)*, right end term, initiation  of
// BoundTables' rounded-down integer terms (fast_tables.hpp).  A pair whose bound is above the cut by the
// margin is finished; every other pair is appended to list 0, unmarked and in both orders when its twin bit is set,
// where the exact stages answer it.  Every decision stays theirs.
//
// Layout: k_pairs_int_list's (thal_pairs_int.hip) -- persistent blocks, batches handed out from a counter and
// counting-sorted by cell count in LDS, lock-step waves of 64 pairs, 64 slots x {value, word} in register tuples with one
// wave-uniform indexed write per cell -- and its FAST visit: the table address is one subtraction of the slot word from a
// per-cell minuend and one unsigned min (LDS image [16 l2 + l1][63 - po], bulge rows filed under the predecessor's po).
// What a cell is here:  min(left end term, min over earlier slots of (T + y + G_pred)),  the pick  min(cell + right end
// term).  No enthalpy, no runner-up, no tie masks, no predecessor bytes, no path, no f64.
// The stacked pair is an ORDINARY ENTRY of the image: row 0 (l1 = l2 = 0) holds g[kWC + a_p * 4 + n1] under the
// predecessor's po, whose n1 field (its 3' neighbour on oligo 1) is the cell's base there; row 0 lies among the l2 = 0
// rows, which take no cell-side term.  No separate stack visit.
#include "int_core.hpp"

namespace msspe {

namespace {

constexpr int kBLThreads = 512;   // two waves per SIMD: the 128 slot registers leave no room for a third (168 VGPRs)
constexpr int kBLBatch = 7;       // passes per sorted batch, as k_pairs_int_list
constexpr int kBLGBase = FastTables::kTSc;   // first compact-table entry kept in LDS: cell-side, end and stack terms
constexpr int kBLGCount = FastTables::kCount - kBLGBase;

// Values (units of 1 / BoundTables::kUnitInv cal/mol): every reachable |value| < kBLReach (build_bound_tables), and every
// cell has a left end term (the stage runs only where pairs_row_tables_ok), so every slot value is a reachable one.
// Void terms are large values, as in the row instance (thal_pairs_row.hip kBndZero ...): a candidate that holds one
// never beats a left end term.
constexpr int kBLReach = BoundTables::kReach;
constexpr int kBLVoidT = 1 << 29;   // a void loop entry, the entry behind the table, the rows a borrow lands on
constexpr int kBLVoidY = 1 << 28;   // a void cell-side term
constexpr int kBLInit = 1 << 27;    // the scan's and the pick's starting minimum
static_assert(kBLInit >= 2 * kBLReach, "above every cell value plus an end term (both below kBLReach)");
static_assert(kBLVoidY - 2 * kBLReach > kBLReach && kBLVoidT - 2 * kBLReach > kBLReach,
              "a candidate that holds a void term (with a reachable slot value and a reachable other term) stays above "
              "every left end term: no cell takes it");
static_assert((long long)kBLVoidT + kBLVoidY + kBLReach < 0x7fffffffLL,
              "largest candidate (void loop + void cell side + reachable slot value) is an int32");
static_assert(-3LL * kBLReach > -0x7fffffffLL, "smallest candidate is an int32");
static_assert(IntTables::kValid > kBLReach, "the tables' void marker is beyond every value");
constexpr unsigned kBLClamp = IntTables::kRows * 256u;   // byte offset of the "not available" entry behind the table
constexpr int kBLEmptyW = 0xff00;                        // coordinates (15, 15): every difference goes negative
static_assert(IntTables::kRows == 14 * 16 + 14 + 1, "rows 16 l2 + l1 with l1, l2 <= 14 are the table's own row count");
static_assert(kSlotsList == 64 && kListStoredMax == kSlotsList - 1, "64 slots, one kept free for the last row's writes");

// ---- the PACKED instance (k_pairs_bound_list_packed): the same minimum on BoundPacked's coarse tables, one register per
// slot -- the packed first stage's arithmetic (thal_pairs_row.hip, "the PACKED bound instance") on this stage's layout.
// The slot word is  W << 15 | (value + bias):  W the 16-bit coordinate word above, whose bits 0 and 1 are zero, so bits
// 15 and 16 of the slot word are zero as in the first stage's  K << 17 | field;  the field is BoundPacked's 15 bits.  The
// cell's minuend carries 0x7fff in its low 15 bits, so  t = C - word  never borrows into the coordinates:  t >> 15  is the
// byte offset into the image, and the low 16 bits of t are  u = 0x7fff - bias - value.  The subtraction SATURATES at 0
// (v_sub_u32 clamp) and the image lies one row down, its row 0 void: a slot whose coordinate difference is negative
// (a column beyond the cell's, the empty word) reads entry 0 with u = 0, and no clamp of the offset is needed -- it is
// at most the minuend's, which lies inside the image.  The minuend's coordinates must not be negative themselves: a cell
// of column 0, which has no predecessor, takes the minuend 0.  A slot of the cell's own row (l1 = -1) lands on a row
// 16 l2 + 15 + 1, void in the image as in the exact-unit instance.  The image holds  Tn = kPLOff - entry  and 0 for void
// or "not available", so  u + Tn - y = kc - (entry + y + value)  with kc = 0x7fff - bias + kPLOff: the running MAXIMUM
// of it is the minimum over the candidates.  64 slot registers instead of 128: the kernel fits 128 VGPRs, i.e. four waves
// per SIMD at 1,024 threads.
// The field: BoundPacked's proven range [lo, hi] does not depend on how many cells a table stores -- it counts a left
// end term plus at most max_k - 1 steps (a chain of 13-mers has at most 13 pairs, whatever the table's size), and a cell
// is at most its left end term -- so it holds for the 53..63 stored cells of this stage as it stands.
constexpr int kPLThreads = 1024;
constexpr int kPLC = kC;            // slots per chunk of the packed scan
constexpr int kPLBatch = kBLBatch;   // passes per sorted batch of the packed instance
constexpr int kPLReach = BoundPacked::kReach;   // every coarse term, every bias and every reachable sum is below this
constexpr int kPLOff = 1 << 28;                 // a real entry is stored as kPLOff - entry (> 0); stored 0: void / not available
constexpr int kPLYVoid = 1 << 26;               // a void cell-side term
constexpr int kPLInit = 1 << 24;                // the pick's starting minimum
static_assert(kPLInit >= 2 * kPLReach, "above every cell value plus an end term");
static_assert((long long)kPLOff - kPLReach - kPLYVoid > 0x7fffLL + kPLReach,
              "a candidate built on a real entry (u + Tn - y, a void cell-side term included) is above every candidate built on "
              "a stored 0 (u - y <= 0x7fff + kPLReach): a 0 is never the maximum beside a real one");
static_assert((long long)kPLOff + kPLReach + 0x7fffLL + kPLReach < 0x7fffffffLL && -(long long)kPLYVoid > -0x7fffffffLL,
              "largest and smallest u + Tn - y are int32s");
static_assert((long long)kPLOff - 3LL * kPLReach > kPLReach,
              "an accumulator that saw stored 0s only (at most 0x7fff + kPLReach) decodes, as kc - acc with bias below kPLReach, "
              "above every left end term");
static_assert(kPLYVoid - 2 * kPLReach > kPLReach, "a candidate that holds a void cell-side term stays above every left end term");
static_assert((long long)0x7fff + kPLOff + kPLYVoid + kPLReach < 0x7fffffffLL, "kc - acc is an int32");
constexpr int kPLEmptyW = kBLEmptyW << 15;   // coordinates (15, 15), field 0: every difference goes negative
static_assert(kPLEmptyW > 0 && ((unsigned)kBLEmptyW << 15) < 0x80000000u, "the empty slot word keeps bit 31 clear");
constexpr int kPLRowShift = 64;              // entries the image lies down by: one void row
// the largest minuend (a lane past its last cell computes on coordinates up to 15): column 15, row 15, po 0
constexpr unsigned kPLMaxOffset = (14u << 12) + (15u << 8) + 252u;
static_assert(kPLMaxOffset < (unsigned)kBLEmptyW, "the empty word is above every minuend: it always saturates");
static_assert(kPLMaxOffset / 4u < IntTables::kRows * 64u + 4u + kPLRowShift, "every offset (at most the minuend's) lies inside the image");

// NT: the block's threads; NB: passes per sorted batch
template <bool PACKED, int NT, int NB>
struct SharedBLT {
    int T[IntTables::kRows * 64 + 4 + (PACKED ? kPLRowShift : 0)];   // + the "not available" entry the clamp lands on (+ the packed instance's void row 0)
    int g[kBLGCount];
    uint2 sorted[NB * NT];
    unsigned hist[256];
    unsigned next_batch;
};
typedef SharedBLT<false, kBLThreads, kBLBatch> SharedBL;
typedef SharedBLT<true, kPLThreads, kPLBatch> SharedPL;

// The LDS image of the loop table: row 16 l2 + l1, column 63 - po (load_tables_int<true>'s), from BoundTables::T, plus
// the stacked pair in row 0.  PACKED: bt holds the coarse terms, and an entry is stored as kPLOff - entry (see kPLOff).
template <bool PACKED, int NT, int NB>
__device__ __forceinline__ void load_tables_bound(SharedBLT<PACKED, NT, NB> &sh, const BoundTables *bt)
{
    for (int e = threadIdx.x; e < IntTables::kRows * 64 + 4; e += NT) {
        const int l2 = e >> 10, l1 = (e >> 6) & 15, po = 63 - (e & 63);
        int v = IntTables::kBig;
        if (e < IntTables::kRows * 64 && l1 <= IntTables::kMaxL) {
            if ((l1 | l2) == 0) {
                v = bt->g[FastTables::kWC + (po & 3) * 4 + ((po >> 2) & 3)];   // a_p, n1 = the cell's base on oligo 1
            } else {
                int pe = po;
                if (l2 == 0) pe = (po & 3) | ((3 - (po >> 4)) << 2);   // a_p | a_c << 2, a_c pairs with the predecessor's n2
                else if (l1 == 0) pe = po & 15;                        // ... a_c is the predecessor's n1
                v = bt->T[(l1 * 16 + l2) * 64 + pe];
            }
        }
        if constexpr (PACKED) sh.T[e + kPLRowShift] = v >= IntTables::kValid ? 0 : kPLOff - v;   // one row down: row 0 is void
        else sh.T[e] = v >= IntTables::kValid ? kBLVoidT : v;
    }
    if (PACKED && threadIdx.x < kPLRowShift) sh.T[threadIdx.x] = 0;
    for (int e = threadIdx.x; e < kBLGCount; e += NT) {
        const int v = bt->g[kBLGBase + e];
        sh.g[e] = v >= IntTables::kValid ? (PACKED ? kPLYVoid : kBLVoidY) : v;   // (only cell-side terms can be void here)
    }
    __syncthreads();
}

// All earlier slots as predecessors of the cell, kC at a time: scan_fill_fast's structure with a plain integer minimum.
template <int PC = 0>
__device__ __forceinline__ void scan_bound(const v32i Ga, const v32i Wa, const v32i Gb, const v32i Wb, int upto, int far_upto,
                                           const char *T, unsigned C, int yTS, int yMM, int &best)
{
    if constexpr (PC * kC < kSlotsList) {
        if (PC * kC < upto) {   // wave-uniform
            unsigned idx[kC];
            int t[kC];
#pragma unroll
            for (int e = 0; e < kC; ++e) idx[e] = min(C - (unsigned)slot_of<64>(Wa, Wb, v8i{}, PC * kC + e), kBLClamp);
#pragma unroll
            for (int e = 0; e < kC; ++e) t[e] = *(const int *)(T + idx[e]);
            if (PC * kC + kC <= far_upto) {   // wave-uniform: every lane has these slots >= 3 rows up (l1 >= 2)
                asm volatile("" ::"n"(PC));   // keeps the chunks from being merged into selects
#pragma unroll
                for (int e = 0; e < kC; ++e) {
                    // rows 0 .. 15 of the image are l2 = 0: a bulge, which takes no cell-side term
                    const int y = idx[e] < 4096u ? 0 : yTS;
                    best = min(best, t[e] + y + slot_of<64>(Ga, Gb, v8i{}, PC * kC + e));
                }
            } else {
                asm volatile("" ::"n"(PC + 64));
#pragma unroll
                for (int e = 0; e < kC; ++e) {
                    const bool bulge = (idx[e] < 4096u) | ((idx[e] & 0xf00u) == 0u);   // l2 == 0 or l1 == 0 (the stacked pair: both)
                    const bool m11 = (idx[e] - 0x1100u) < 256u;                      // l1 == l2 == 1
                    const int y = bulge ? 0 : (m11 ? yMM : yTS);
                    best = min(best, t[e] + y + slot_of<64>(Ga, Gb, v8i{}, PC * kC + e));
                }
            }
            scan_bound<PC + 1>(Ga, Wa, Gb, Wb, upto, far_upto, T, C, yTS, yMM, best);
        }
    }
}

// The minimum over the lane's cells of (cell value + right end term); kBLInit: the lane has no cell.  n_cells counts
// every complementary cell (0: idle lane); the cells of the lane's last row may lie beyond slot 62: they are computed
// and may be picked, and all land in slot 63, which nothing reads (run_pair_int's rule: wave_bound sizes the table).
__device__ __forceinline__ int run_pair_bound_list(const SharedBL &sh, const SeqPair &q, unsigned rowmask, int n_cells, int nmax)
{
    v32i Ga = 0, Wa = kBLEmptyW, Gb = 0, Wb = kBLEmptyW;
    CellCtx c;
    unsigned Rrem = rowmask, mrem = 0;
    int im1 = 0, jm1 = 0;
    // first slot of the lane's current row and of its two previous non-empty rows: every slot below row_lo2 lies at
    // least three rows above the current cell
    int row_lo0 = 0, row_lo1 = 0, row_lo2 = 0;
    int pick = kBLInit;
    for (int slot_ = 0; slot_ < nmax; ++slot_) {
        const int slot = __builtin_amdgcn_readfirstlane(slot_);
        // ---- next complementary cell in row-major order (as run_pair_int)
        const bool newrow = mrem == 0;
        const int t = __ffs((int)Rrem) - 1;
        const int a_new = (q.s1 >> (t & 31)) & 3;
        const unsigned m_new = spaced_mask(q.s2, 3 - a_new, q.lenmask);
        im1 = newrow ? (t >> 1) : im1;
        row_lo2 = newrow ? row_lo1 : row_lo2;
        row_lo1 = newrow ? row_lo0 : row_lo1;
        row_lo0 = newrow ? slot : row_lo0;
        Rrem = newrow ? (Rrem & (Rrem - 1)) : Rrem;
        mrem = newrow ? m_new : mrem;
        jm1 = (__ffs((int)mrem) - 1) >> 1;
        mrem &= mrem - 1;
        im1 &= 15;
        jm1 &= 15;
        const CellBases b = cell_bases(q, im1, jm1, c);
        const bool in = slot < n_cells;   // lanes past their last cell compute garbage (every address stays in range)
        const int far_upto = wave_min_64(in ? row_lo2 : 63);
        const unsigned C = (unsigned)(((jm1 - 1) << 12) + ((im1 - 1) << 8) + 252);
        int best = kBLInit;
        scan_bound<>(Ga, Wa, Gb, Wb, slot, far_upto, (const char *)sh.T, C, sh.g[c.yTS - kBLGBase], sh.g[c.yMM - kBLGBase], best);
        const int G0 = min(sh.g[b.idxL - kBLGBase], best);
        pick = in ? min(pick, G0 + sh.g[b.idxR - kBLGBase]) : pick;
        const int Wcell = (jm1 << 12) | (im1 << 8) | (b.po_c << 2);
        // ---- publish the cell: one indexed write per plane over the whole 64-register plane (run_pair_int's, list mode)
        const int ps = min(slot, kSlotsList - 1);   // wave-uniform
        asm volatile("s_set_gpr_idx_on %[SLOT], gpr_idx(DST)\n\t"
                     "v_mov_b32 v120, %[G]\n\t"
                     "v_mov_b32 v184, %[W]\n\t"
                     "s_set_gpr_idx_off"
                     : "+{v[120:151]}"(Ga), "+{v[152:183]}"(Gb), "+{v[184:215]}"(Wa), "+{v[216:247]}"(Wb)
                     : [G] "v"(G0), [W] "v"(Wcell), [SLOT] "s"(ps)
                     : "m0");
    }
    return pick;
}

// ---- the packed instance's cell loop
// the low 16 bits of t (u: bit 15 is zero) added to the image's entry: one instruction
__device__ __forceinline__ int add_low16(unsigned t, int tn)
{
    int r;
    asm("v_mad_u32_u16 %0, %1, 1, %2" : "=v"(r) : "v"(t), "v"(tn));
    return r;
}

// scan_bound on the packed words: acc = max(acc, u + Tn - y) over all earlier slots (see kPLOff).
template <int PC = 0>
__device__ __forceinline__ void scan_bound_packed(const v32i Wa, const v32i Wb, int upto, int far_upto, const char *T, unsigned C,
                                                  int yTS, int yMM, int &acc)
{
    if constexpr (PC * kPLC < kSlotsList) {
        if (PC * kPLC < upto) {   // wave-uniform
            unsigned t[kPLC], idx[kPLC];
            int tn[kPLC];
#pragma unroll
            for (int e = 0; e < kPLC; ++e) {
                t[e] = __builtin_elementwise_sub_sat(C, (unsigned)slot_of<64>(Wa, Wb, v8i{}, PC * kPLC + e));
                idx[e] = t[e] >> 15;
            }
#pragma unroll
            for (int e = 0; e < kPLC; ++e) tn[e] = *(const int *)(T + idx[e]);
            if (PC * kPLC + kPLC <= far_upto) {   // wave-uniform: every lane has these slots >= 3 rows up (l1 >= 2)
                asm volatile("" ::"n"(PC));   // keeps the chunks from being merged into selects
#pragma unroll
                for (int e = 0; e < kPLC; ++e) {
                    // rows 0 .. 15 of the image are l2 = 0: a bulge, which takes no cell-side term
                    const int y = idx[e] < 4096u ? 0 : yTS;
                    acc = max(acc, add_low16(t[e], tn[e]) - y);
                }
            } else {
                asm volatile("" ::"n"(PC + 64));
#pragma unroll
                for (int e = 0; e < kPLC; ++e) {
                    // the image's row is 16 l2 + l1 + 1: bits 12.. hold l2 and bits 8 .. 11 l1 + 1 wherever l1 <= 14 (l1 = 15,
                    // a slot of the cell's own row, carries into l2: those rows are void, whatever term they are given)
                    const bool bulge = (idx[e] < 4096u) | ((idx[e] & 0xf00u) == 0x100u);   // l2 == 0 or l1 == 0 (the stacked pair: both)
                    const bool m11 = (idx[e] & 0xff00u) == 0x1200u;                       // l1 == l2 == 1
                    const int y = bulge ? 0 : (m11 ? yMM : yTS);
                    acc = max(acc, add_low16(t[e], tn[e]) - y);
                }
            }
            scan_bound_packed<PC + 1>(Wa, Wb, upto, far_upto, T, C, yTS, yMM, acc);
        }
    }
}

// run_pair_bound_list on the packed table: the same cells in the same order, the same slot for each, in coarse units;
// kPLInit: the lane has no cell.  bias: BoundPacked::bias (wave-uniform).
__device__ __forceinline__ int run_pair_bound_list_packed(const SharedPL &sh, const SeqPair &q, unsigned rowmask,
                                                          int n_cells, int nmax, int bias)
{
    v32i Wa = kPLEmptyW, Wb = kPLEmptyW;
    CellCtx c;
    unsigned Rrem = rowmask, mrem = 0;
    int im1 = 0, jm1 = 0;
    int row_lo0 = 0, row_lo1 = 0, row_lo2 = 0;   // as run_pair_bound_list
    const int kc = 0x7fff - bias + kPLOff;       // u + Tn - y = kc - (entry + y + predecessor's value)
    int pick = kPLInit;
    for (int slot_ = 0; slot_ < nmax; ++slot_) {
        const int slot = __builtin_amdgcn_readfirstlane(slot_);
        // ---- next complementary cell in row-major order (as run_pair_int)
        const bool newrow = mrem == 0;
        const int t = __ffs((int)Rrem) - 1;
        const int a_new = (q.s1 >> (t & 31)) & 3;
        const unsigned m_new = spaced_mask(q.s2, 3 - a_new, q.lenmask);
        im1 = newrow ? (t >> 1) : im1;
        row_lo2 = newrow ? row_lo1 : row_lo2;
        row_lo1 = newrow ? row_lo0 : row_lo1;
        row_lo0 = newrow ? slot : row_lo0;
        Rrem = newrow ? (Rrem & (Rrem - 1)) : Rrem;
        mrem = newrow ? m_new : mrem;
        jm1 = (__ffs((int)mrem) - 1) >> 1;
        mrem &= mrem - 1;
        im1 &= 15;
        jm1 &= 15;
        const CellBases b = cell_bases(q, im1, jm1, c);
        const bool in = slot < n_cells;   // lanes past their last cell compute garbage (every address stays in range)
        const int far_upto = wave_min_64(in ? row_lo2 : 63);
        // column 0 has no predecessor and its coordinate difference would start below zero: minuend 0, every slot saturates.
        // (im1 << 8: row im1 - 1 of run_pair_bound_list's minuend and the one row the image lies down by)
        const unsigned C = jm1 == 0 ? 0u : ((unsigned)(((jm1 - 1) << 12) + (im1 << 8) + 252) << 15) | 0x7fffu;
        int acc = 0;   // below every candidate built on a real entry: decodes far above the left end term
        scan_bound_packed<>(Wa, Wb, slot, far_upto, (const char *)sh.T, C, sh.g[c.yTS - kBLGBase], sh.g[c.yMM - kBLGBase], acc);
        const int G0 = min(sh.g[b.idxL - kBLGBase], kc - acc);
        pick = in ? min(pick, G0 + sh.g[b.idxR - kBLGBase]) : pick;
        // G0 + bias is a 15-bit field: BoundPacked's proven range of every publishable value (a lane past its last cell
        // publishes the empty word)
        const int Wcell = in ? (int)((unsigned)((jm1 << 12) | (im1 << 8) | (b.po_c << 2)) << 15) + (G0 + bias) : kPLEmptyW;
        // ---- publish the cell: one indexed write over the whole 64-register plane
        const int ps = min(slot, kSlotsList - 1);   // wave-uniform
        asm volatile("s_set_gpr_idx_on %[SLOT], gpr_idx(DST)\n\t"
                     "v_mov_b32 v64, %[W]\n\t"
                     "s_set_gpr_idx_off"
                     : "+{v[64:95]}"(Wa), "+{v[96:127]}"(Wb)
                     : [W] "v"(Wcell), [SLOT] "s"(ps)
                     : "m0");
    }
    return pick;
}

// One lock-step pass of the wave: lane = one entry of U.  Every exit is wave-uniform (the batch loop's barriers and the
// callers' counter fetches depend on it).
// PACKED: the packed instance's cell loop and units (a.bt: BoundPacked::q); everything around it is the same.
template <bool PACKED, int NT, int NB>
__device__ __forceinline__ void wave_bound(const SharedBLT<PACKED, NT, NB> &sh, const IntArgs &a, int row, int col, bool twin, bool inside)
{
    const int lane = threadIdx.x & 63;
    SeqPair q;
    unsigned rowmask;
    const uint64_t pa = a.f.pool[inside ? row : 0], pb = a.f.pool[inside ? col : 0];
    int n_cells = setup_pair(pa, pb, a.f.k, q, rowmask);
    const bool sym = self_complementary(pa, a.f.k) && self_complementary(pb, a.f.k);
    const int last_row = __popc(spaced_mask(q.s2, 3 - (int)((q.s1 >> (2 * (a.f.k - 1))) & 3u), q.lenmask));
    // The first stage sends nothing here that this table cannot hold, and no pair of two self-complementary oligos; an
    // entry that is one all the same is passed on unbounded, like a survivor.
    const bool pass_on = inside & ((n_cells - last_row > kListStoredMax) | sym);
    const bool active = inside & !pass_on & (n_cells > 0);
    if (!active) n_cells = 0;
    const int nmax = wave_max_u8(n_cells);
    constexpr int kInit = PACKED ? kPLInit : kBLInit;
    int pick = kInit;
    if (nmax != 0) {   // wave-uniform
        if constexpr (PACKED) pick = run_pair_bound_list_packed(sh, q, rowmask, n_cells, nmax, __builtin_amdgcn_readfirstlane(a.packed_bias));
        else pick = run_pair_bound_list(sh, q, rowmask, n_cells, nmax);
    }
    const int lb = pick + a.bt->init;   // a lane without a chain keeps kBLInit (kPLInit): above every cut
    if (a.bound_plane) {
        if (inside & !pass_on)
            a.bound_plane[(size_t)(row - a.f.sinks.row0) * (size_t)a.f.sinks.ncols + (size_t)(col - a.f.sinks.col0)] =
                pick >= kInit ? INFINITY : PACKED ? (double)lb * a.packed_unit : (double)lb / BoundTables::kUnitInv;
        return;
    }
    const bool out = pass_on | (active & (lb <= a.bt->cut));   // a culled pair is finished: it writes nothing
    const bool both = twin & (row != col);
    if (a.bound_list_stats) {
        const unsigned long long m1 = __ballot(out), m2 = __ballot(out & both);
        if (lane == 0 && m1) atomicAdd(&a.bound_list_stats[1], (unsigned long long)(__popcll(m1) + __popcll(m2)));
    }
    if (out) {   // unmarked: the exact integer list stage retries it
        const uint32_t at = atomicAdd(a.f.ovf_count, both ? 2u : 1u);
        if (at < a.f.ovf_cap) a.f.ovf_list[at] = make_uint2((unsigned)row, (unsigned)col);
        if (both && at + 1u < a.f.ovf_cap) a.f.ovf_list[at + 1u] = make_uint2((unsigned)col, (unsigned)row);
    }
}

// The block's work: NT threads, batches of depth x NT entries, depth <= NB.  (a by value, as the kernels take it: by
// reference the exact-unit instance's scalar code comes out differently allocated.)
template <bool PACKED, int NT, int NB>
__device__ __forceinline__ void bound_list_block(SharedBLT<PACKED, NT, NB> &sh, const IntArgs a, uint2 *u_list)
{
    if (*a.f.in_count == 0u) return;   // an empty list: no table loads
    load_tables_bound(sh, a.bt);
    const long n_work = (long)min(*a.f.in_count, a.f.ovf_cap);
    if (a.bound_list_stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.bound_list_stats[0], (unsigned long long)n_work);
    // batches of depth x NT entries, sorted together and run as `depth` lock-step passes (k_pairs_int_list's rule: a
    // short list is spread over all the blocks).  Which pairs are culled does not depend on the depth.
    const long per_pass = (long)gridDim.x * NT;
    const int depth = (int)min((long)NB, max(1L, (n_work + per_pass - 1) / per_pass));
    const long batch = (long)depth * NT;
    const long n_batches = (n_work + batch - 1) / batch;
    for (;;) {
        if (threadIdx.x == 0) sh.next_batch = atomicAdd(a.work_counter, 1u);
        for (int e = threadIdx.x; e < 256; e += NT) sh.hist[e] = 0u;
        __syncthreads();
        const long bt = (long)sh.next_batch;
        if (bt >= n_batches) break;   // block-uniform
        uint2 mine[NB];
        int key[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const long w = bt * batch + (long)j * NT + threadIdx.x;
            const bool inside = (j < depth) & (w < n_work);   // passes beyond the depth hold padding only
            mine[j] = inside ? u_list[w] : make_uint2(0xffffffffu, 0u);
            int nc = 255;   // padding sorts last
            if (inside) {
                SeqPair q;
                unsigned rowmask;
                nc = min(setup_pair(a.f.pool[mine[j].x & ~(kNeedsF64 | kListTwin)], a.f.pool[mine[j].y], a.f.k, q, rowmask), 254);
            }
            key[j] = nc;
            atomicAdd(&sh.hist[nc], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {   // exclusive scan of the 256 bins
            unsigned v[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = sh.hist[threadIdx.x * 4 + q];
                sum += v[q];
            }
            unsigned incl = sum;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned up = __shfl_up(incl, off);
                if ((int)threadIdx.x >= off) incl += up;
            }
            unsigned run = incl - sum;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sh.hist[threadIdx.x * 4 + q] = run;
                run += v[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NB; ++j) sh.sorted[atomicAdd(&sh.hist[key[j]], 1u)] = mine[j];
        __syncthreads();
        const long n_own = min(batch, n_work - bt * batch);
        for (int j = 0; j < depth; ++j) {
            const long e = (long)j * NT + threadIdx.x;
            const bool inside = e < n_own;
            const uint2 pr = sh.sorted[inside ? e : 0];
            wave_bound(sh, a, (int)(pr.x & ~(kNeedsF64 | kListTwin)), (int)pr.y, (pr.x & kListTwin) != 0u, inside);
        }
        __syncthreads();   // every wave is done with the sorted batch (and has read next_batch) before the next one
    }
}

__global__ void __launch_bounds__(kBLThreads) k_pairs_bound_list(IntArgs a, uint2 *u_list)
{
    __shared__ SharedBL sh;
    bound_list_block(sh, a, u_list);
}

// The packed instance: a.bt holds BoundPacked::q, a.packed_bias its bias (launch_pairs_bound_list).
__global__ void __launch_bounds__(kPLThreads) k_pairs_bound_list_packed(IntArgs a, uint2 *u_list)
{
    __shared__ SharedPL sh;
    bound_list_block(sh, a, u_list);
}

}  // namespace

hipError_t launch_pairs_bound_list(const PairKernelArgs &a, const BoundTables *bt, uint2 *u_list, const uint32_t *u_count,
                                   unsigned long long *stats, double *bound_plane, int n_cu, hipStream_t stream,
                                   const BoundTables *packed_q, int packed_bias, int packed_shift)
{
    if (a.k > 13 || a.k < 2 || !bt || !u_list || !u_count || (!bound_plane && (!a.overflow_list || !a.overflow_count)))
        return hipErrorInvalidValue;
    // packed_q: BoundPacked::q on the device -- the packed instance runs (same contract, coarse units)
    if (packed_q && (packed_shift < BoundPacked::kShiftMin || packed_shift > BoundPacked::kShiftMax || packed_bias < 0 ||
                     packed_bias >= BoundPacked::kReach))
        return hipErrorInvalidValue;
    IntArgs x;
    FastArgs &f = x.f;
    f.ft = a.ft;
    f.c = a.c;
    f.pool = a.pool;
    f.cols_sorted = nullptr;
    f.perm = nullptr;
    f.k = a.k;
    f.row0 = a.row0;
    f.row1 = a.row1;
    f.col0 = a.col0;
    f.col1 = a.col1;
    f.sinks = a.sinks;
    f.ovf_list = a.overflow_list;
    f.ovf_count = a.overflow_count;
    f.ovf_cap = a.overflow_cap;
    f.in_list = u_list;
    f.in_count = u_count;
    x.it = nullptr;
    x.reasons = nullptr;
    x.stat_off = 0;
    x.work_counter = a.work_counter;
    x.bt = bt;
    x.bound_plane = bound_plane;
    x.bound_list_stats = stats;
    if (hipError_t e = hipMemsetAsync(a.work_counter, 0, sizeof(unsigned), stream); e != hipSuccess) return e;
    if (packed_q) {
        x.bt = packed_q;
        x.packed_bias = packed_bias;
        x.packed_unit = (double)(1 << (packed_shift - BoundPacked::kShiftMin));
        hipLaunchKernelGGL(k_pairs_bound_list_packed, dim3(n_cu), dim3(kPLThreads), 0, stream, x, u_list);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_pairs_bound_list, dim3(n_cu), dim3(kBLThreads), 0, stream, x, u_list);
    return hipGetLastError();
}

}  // namespace msspe
