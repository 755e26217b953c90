// fast_tables.hpp -- LDS-resident tables of the tuned all-pairs kernel (thal_pairs.hip).
//
// One flat array of entries (S: double, H: int32, same index in both planes).  The candidate of a
// bulge / interior loop closed by predecessor p and cell c is, in Primer3's operation order
// (thal.c calc_bulge_internal):
//      S = (((L + X) + Y) + Z) + S_p        H = L_H + X_H + Y_H + H_p
// Everything that does not depend on BOTH p and c is folded on the host with the very same
// IEEE-754 additions, in the same order, that the kernel would otherwise execute:
//      kind        first gather (index)                              second gather     third
//      interior    NB[sz][po]   = interior[sz-1] + tstack[po]        TSc[ci]           ZT[l1-l2]
//      1 x 1       NB[2][po]    = stackmm[po]  (interior row 2 is otherwise unused)   MMc[ci]   ZT[0]
//      bulge >= 2  BU[a_c][sz][a_p] = (bulge[sz-1] + AT(a_p)) + AT(a_c)                ZERO      ZERO
//      bulge 1     BU[a_c][1][a_p]  = bulge[0] + stack[a_p][a_c]  (*)                   ZERO      ZERO
//      (stack)     BU[a_c][0][a_p]  = not available: the stacked pair is not a loop candidate
//  (*) thal.c rejects a single-base bulge whose own (S,H) has H > 0 or S > 0 before the
//      predecessor is added; that test is applied here once per table entry.
// ZT[d] = ILAS * |d| exactly as the kernel would multiply it (ILAS * 0 is -0.0 and stays so);
// adding the ZERO entry (+0.0) is an exact no-op, so all kinds share one formula.
// po = a_p | s1[ii+1] << 2 | s2[jj+1] << 4 ; ci = (s2[j] * 4 + s2[j-1]) * 4 + s1[i-1].
#pragma once

#include <cstdint>

#include "nn_params.hpp"

namespace msspe {

struct FastTables {
    static constexpr int kMaxSz = 28;                          // loop sizes 0..28 (= 2 * 16 - 4) are addressable
    static constexpr int kNB = 0;                              // [sz-2][po], sz = 2..28: 27 * 64
    static constexpr int kBU = kNB + (kMaxSz - 1) * 64;        // [a_c][sz][a_p], sz = 0..28: 4 * 29 * 4
    static constexpr int kBUStride = (kMaxSz + 1) * 4;
    static constexpr int kTSc = kBU + 4 * kBUStride;           // [ci] 64
    static constexpr int kMMc = kTSc + 64;                     // [ci] 64
    static constexpr int kZero = kMMc + 64;                    // 1 (+3 pad)
    static constexpr int kZT = kZero + 4;                      // [32 + (l1 - l2)], 64 entries
    static constexpr int kEndL = kZT + 64;                     // [a*25 + oa*5 + ob]  100
    static constexpr int kEndR = kEndL + 100;                  // 100
    static constexpr int kWC = kEndR + 100;                    // [x*4 + y]       16
    static constexpr int kCount = kWC + 16;
    double S[kCount];
    int32_t H[kCount];
    int32_t usable;      // 1 when the kernel's exactness preconditions hold (see build_fast_tables)
    int32_t max_k;       // largest oligo length the preconditions were verified for
};

// Preconditions checked here (else usable = 0 and the caller must use the generic kernel):
//   * every finite enthalpy is an integer multiple of 10 cal/mol (packed as H/10 in 18 bits);
//   * no accepted value can reach the MinEntropyCutoff clamp for oligos up to max_k bases;
//   * 2 * max_k - 4 <= kMaxSz (every loop an oligo pair can form has a table row).
bool build_fast_tables(const NNTables &t, const PairTables &pt, int max_k, FastTables &out);

// Integer image of the same tables for the exact-integer kernel (thal_pairs_int.hip).
// Every table entropy is a multiple of 0.01 e.u. and every enthalpy a multiple of 10 cal/mol, and
// the interior-loop asymmetry term is ILAS * |l1 - l2| with 310.15 * ILAS = -300 exactly, so the
// value of a DP cell is the integer triple (h = H / 10, s = 100 * S_tables, n = sum |l1 - l2|) and
//      2000 * dG(37 C) = 20000 h + 600000 n - 6203 s         (dG = H - 310.15 S)
// is an exact int32.  Primer3 compares dG values as doubles; two candidates whose exact values
// differ are at least 5e-4 cal/mol apart, far beyond double rounding, so integer comparison
// gives the same answer.  Exact ties (where double rounding decides) are detected and those
// pairs are handed to the f64 kernel.
struct IntTables {
    static constexpr int kMaxL = 14;                       // l1, l2 <= k - 2
    static constexpr int kRows = kMaxL * 17 + 1;           // row d = l1 * 16 + l2
    // "not available" is a large value, not a flag.  A candidate is the sum of a loop entry, a
    // cell-side entry and the predecessor's value: two unavailable terms must not wrap
    // (2 kBig + kReach < 2^31) and a single one must land above kValid (kBig - kReach >= kValid),
    // where kReach bounds every reachable |value| (checked by build_int_tables).
    static constexpr int32_t kBig = 900000000;             // not available
    static constexpr int32_t kValid = 500000000;           // candidates at or above this are void
    static constexpr int32_t kReach = 300000000;
    static constexpr int32_t kGh = 20000, kGn = 600000, kGs = 6203;
    // loop term of predecessor p -> cell c without the cell-side mismatch term:
    //   interior / 1x1 : column po (fast_tables.hpp), asymmetry included
    //   bulge          : column a_p | a_c << 2
    //   d = 0 (stack)  : kBig, the stacked pair is not a loop candidate
    int32_t T[kRows * 64];
    int32_t g[FastTables::kCount];   // kGh * (H / 10) - kGs * s per FastTables entry (kBig: unavailable)
    int32_t s[FastTables::kCount];   // round(100 * S)
    int32_t usable, max_k;
};
// usable = 0 unless every finite entropy is a multiple of 0.01 within 1e-7 and the packed fields
// (s: 18 bits signed, sums below kValid) cannot overflow for oligos up to max_k bases.
bool build_int_tables(const FastTables &ft, int max_k, IntTables &out);

// Tables of the BOUND first stage (thal_pairs_row.hip k_pairs_bound): every term as its free energy at the
// temperature dG is reported at, g = H - temp_k * S, in integer units of 1 / kUnitInv cal/mol, ROUNDED DOWN.  A
// structure thal() can report is a chain  left end term, (stacked pair | loop)*, right end term, initiation, and its
// dG = dH - temp_k (dS + N salt) with N = pairs - 1 is the sum of its terms' g where every step from one pair to the
// next also carries - temp_k * salt.  The plain minimum over all chains of the rounded-down terms is therefore a lower
// bound of every dG thal() can report, whatever maxTM(), the acceptance rules and the traceback select.
struct BoundTables {
    static constexpr int kUnitInv = 64;                    // units per cal/mol
    // Exactness margin of the cull rule, in units (= 1 cal/mol): a pair is culled iff bound > g_cut + kMargin.  The
    // rounding of the terms only lowers the bound (soundness needs none of the margin); what the margin covers is
    // the distance between the real-number sum and what thal() prints: its f64 roundings (< 1e-8 cal/mol) and the
    // traceback's 1e-5 e.u. equality tolerance per step (13 steps x 1e-5 x 373.15 K < 0.05 cal/mol).
    static constexpr int kMargin = kUnitInv;
    static constexpr int32_t kReach = 1 << 26;             // bounds every reachable |value| (checked by build_bound_tables)
    // The mirrored first stage (square same-pool screens) uses the bound of (a, b) for (b, a) as well.  Swapping the strands
    // maps every chain of (a, b) onto a chain of (b, a) whose terms are the swapped partners of its own; bound_mirror_ok()
    // admits a table set only if every term equals its partner within kMirrorTol (real values, before rounding).  A
    // chain of 13-mers has at most kMirrorTerms terms (2 end terms, 12 steps of at most 2, the initiation), so
    //      LB(a, b) <= RB(a, b) <= RB(b, a) + kMirrorTerms kMirrorTol <= dG(b, a) + 27e-6     (RB: the real-number minimum)
    // and that slack, too, comes out of the margin.
    static constexpr double kMirrorTol = 1e-6;             // cal/mol
    static constexpr int kMirrorTerms = 27;
    static_assert(13 * 1e-5 * 373.15 + 1e-6 + kMirrorTerms * kMirrorTol < (double)kMargin / kUnitInv,
                  "the margin covers the traceback's tolerance and the mirror's");
    // "not available" as in IntTables (kBig; anything at or above kValid is void)
    int32_t T[IntTables::kRows * 64];    // loop term of IntTables::T's layout: asymmetry and the step's salt term included
    int32_t g[FastTables::kCount];       // cell-side and end terms as they are; kWC: the stacked pair WITH the step's salt term
    int32_t init;                        // duplex initiation
    int32_t cut;                         // cull iff init + min over chains > cut: floor((g_cut + margin) * kUnitInv)
    int32_t usable, max_k;
    int32_t mirror_ok;                   // bound_mirror_ok(): the bound of (a, b) may stand for (b, a)
};
// The exact values the integers above round down, for the tests: g of FastTables entry e (salt_steps: 0 or 1 salt
// terms added), +inf where the tables hold none.
double bound_term_exact(const FastTables &ft, const ThalConsts &c, int e, int salt_steps);
// usable = 0 unless every reachable sum of max_k pairs stays below kReach, temp_k is within 0 .. 100 C and g_cut <= 0.
bool build_bound_tables(const FastTables &ft, const ThalConsts &c, int max_k, BoundTables &out);
// Every real-valued term the bound recurrence can use equals its strand-swapped partner within kMirrorTol (void entries
// mirror void ones): left end <-> right end of the swapped context, stacked pair <-> the stack read from the other
// strand, bulge and interior loops (l1, l2) <-> (l2, l1) with closing pairs and mismatch neighbours swapped, the
// cell-side mismatch terms kTSc / kMMc <-> the predecessor-side terms they become.
bool bound_mirror_ok(const FastTables &ft, const ThalConsts &c);

// Tables of the PACKED bound first stage (thal_pairs_row.hip k_pairs_bound_packed): BoundTables' terms in a coarser
// unit of 2^(shift - 6) cal/mol (shift 6, 7 or 8: 1, 2 or 4 cal/mol), every finite term FLOORED (arithmetic >> shift;
// void stays void), so that a cell value fits the 15-bit field of the slot word beside K and the slot table is one
// register per slot.  floor(a) + floor(b) <= floor(a + b): the minimum over chains of the floored terms, times the
// unit, is at most BoundTables' minimum, hence a lower bound of every dG thal() can report all the same -- coarser
// rounding costs survivors, never soundness.  The cut is floor(cut / 2^shift) and the cull rule  lbq > cutq, which
// implies lbq 2^shift >= (cutq + 1) 2^shift > cut: the margin is spent exactly as before.
struct BoundPacked {
    static constexpr int kFieldBits = 15;
    static constexpr int32_t kFieldMax = (1 << kFieldBits) - 1;
    static constexpr int kShiftMin = 6, kShiftMax = 8;     // 2^6 units of 1/64 cal/mol = 1 cal/mol
    static_assert((1 << kShiftMin) == BoundTables::kUnitInv, "shift 6 is 1 cal/mol");
    // every coarse term and every reachable coarse sum is below this (BoundTables::kReach >> kShiftMin): the kernel's
    // "not available" arithmetic is stated against it
    static constexpr int32_t kReach = BoundTables::kReach >> kShiftMin;
    BoundTables q;       // g, T, init, cut in coarse units (usable, max_k, mirror_ok copied)
    int32_t shift;       // 0 when unusable
    int32_t bias;        // slot field = cell value + bias
    int32_t lo, hi;      // PROVEN range of every value a cell can publish, coarse units: lo + bias >= 0, hi + bias <= kFieldMax
    int32_t usable;
};
// From finished BoundTables: the smallest shift whose proven range of publishable cell values fits the field.  A cell's
// value is min(left end term, candidates), so it is at most the largest finite left end term; and it is the sum of a
// left end term and at most max_k - 1 steps, a step being a table entry (loop or stacked pair) plus at most one
// cell-side term, so it is at least the most negative left end term plus (max_k - 1) x the most negative step.
// usable = 0 (and the exact-unit instance runs) when bt is unusable or no shift fits.
bool build_bound_packed(const BoundTables &bt, int max_k, BoundPacked &out);

// Constants of the WINDOWED packed instance (thal_pairs_row.hip k_pairs_bound_window): a cell of row i scans the rows
// i-F .. i-1 exactly and takes ONE candidate for every row above them,  farmin + min(bfar, ifar + cell-side term),
// farmin being the smallest value of any stored cell of those rows.  ifar / bfar: the smallest finite coarse entry of
// BoundPacked::q.T over the rows l1 >= F with l2 >= 1 / with l2 = 0, any context -- at most the entry of every real
// predecessor up there, so the relaxed value is at most the packed instance's and a lower bound all the same.  The proven
// range holds as it is: the far step is not below the most negative step, a chain still has at most max_k - 1 steps, and a
// cell is still at most its left end term.
struct BoundWindow {
    int32_t F;                // rows of the window
    int32_t ifar, bfar;       // coarse units; kVoid: no finite entry (the candidate loses that branch, or is void altogether)
    int32_t usable;           // 0 wherever the packed instance is unusable, or a real field could be kFieldMax (farmin's "no cell")
    static constexpr int32_t kVoid = 1 << 26;   // thal_pairs_row.hip kWinVoid
};
bool build_bound_window(const BoundPacked &bp, int F, BoundWindow &out);

}  // namespace msspe
