// capi.cpp -- extern "C" boundary of libmsspe_hip.so (declared in include/msspe_hip.h).
//
// Each entry point replaces one process boundary or stage-A function of the reference:
//   msspe_cross_dimer*     run_ntthal            /root/reference/od-msspe/src/delta_g.rs:83-153
//   msspe_oligo_stats*     check_primers         /root/reference/od-msspe/src/primer.rs:143-166
//   msspe_kmer_candidates* get_segment_manager + find_candidates_kmers  src/main.rs:196-235,331-406
//   msspe_conflict_cover*  vertex_cover (the greedy cover of the conflict graph)  src/main.rs:754-798
//   msspe_conflict_tubes*  (engine extension) the same graph split into reaction tubes instead of covered
// There is no CPU fallback: every compute entry point needs a gfx950 device.
#include "../../include/msspe_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "conflict_cover.hpp"
#include "conflict_graph.hpp"
#include "background.hpp"
#include "background_thal.hpp"
#include "background_amplicons.hpp"
#include "stream_reach.hpp"
#include "panel_thin_reach.hpp"
#include "coverage_mm.hpp"
#include "coverage_thal.hpp"
#include "kernels.hpp"
#include "kmer_stage.hpp"
#include "nn_params.hpp"
#include "thal_dense.hpp"
#include "panel_select.hpp"
#include "panel_thin.hpp"
#include "panel_thin_thal.hpp"
#include "screen_plan.hpp"
#include "slab_split.hpp"
#include "tube_split.hpp"

using namespace msspe;

namespace {

struct ChemEntry {
    msspe_chem chem;
    float threshold;
    int kind = 0;                 // kCutAnyDg: c[].g_cut = g_cut(threshold); kCutEndT (the END screen's entry) and
                                  // kCutAnyT (ANY site scores of msspe_background_thal*): t_cut(threshold)
    ThalConsts c[2];
    PairTables *d_pt = nullptr;   // 2 entries: ordinary, both self-complementary
    FastTables *d_ft = nullptr;   // tables of the tuned all-pairs kernel (ordinary pairs)
    bool fast_ok = false;
    IntTables *d_it = nullptr;    // integer image for the exact-integer kernel
    bool int_ok = false;
    bool row_ok = false;          // ... and the row-specialised kernel (thal_pairs_row.hip)
    BoundTables *d_bt = nullptr;  // the bound first stage's tables (thal_pairs_row.hip k_pairs_bound)
    bool bound_ok = false;        // ... usable: row_ok, g_cut <= 0, values in range (build_bound_tables)
    bool mirror_ok = false;       // ... and strand-symmetric term by term (bound_mirror_ok): a square screen fills each unordered pair once
    BoundTables *d_btq = nullptr; // the packed bound instance's coarse tables (BoundPacked::q; k_pairs_bound_packed)
    bool packed_ok = false;       // ... usable: a proven range of every cell value fits the slot word's 15-bit field (build_bound_packed)
    int packed_shift = 0, packed_bias = 0;
    BoundWindow window{};         // the windowed packed instance's constants (build_bound_window; k_pairs_bound_window)
    bool window_ok = false;       // ... usable: packed_ok, and no real slot field equals the far minimum's "no cell"
    // option pair_bound = auto: the share of pairs the bound stage could not cull, per oligo length, as the first
    // call's probe launch measured it (this entry keys on chemistry AND threshold); < 0: no record yet
    float bound_share[16] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    SplitTables *d_st = nullptr;  // long oligos (thal_pairs_split.hip)
    int split_max_k = 0;          // 0: not usable
    int wave_max_k = 0;           // f64 one-wave-per-pair kernel (thal_pairs_wave.hip)
};

constexpr int kCutAnyDg = 0, kCutEndT = 1, kCutAnyT = 2;   // ChemEntry::kind: one cache entry per kind, chemistry and threshold
constexpr int kHairpinLaneFrom = 8192;       // oligos per call from which HAIRPIN_TH runs one lane per oligo (msspe_oligo_stats_dev)
constexpr long kListCapMin = 1L << 20;       // hand-over list entries (grows with the call up to kListCapMax): one launch can never overrun it
constexpr long kListCapMax = 1L << 30;       // 8 GB per list (two of them, 6 % of the card's memory): the stages behind the first
                                             // run every two launches of 2^29 pairs, so that a list cannot be overrun even if
                                             // every pair were handed on (2.7 % are); k_accumulate_overflow checks the counters
                                             // against it all the same.  The small kernels of a flush do not fill the card:
                                             // 2^28 -> 2^30 is 17 -> 5 flushes per 65,536^2 screen and 1.5 % of its time
constexpr size_t kGenericLanes = 1u << 16;   // lanes of the generic kernels' workspace
constexpr int kOvfTotals = 2 + 7;            // msspe_ctx::d_ovf_total: two flags / totals, then one total per hand-over list
constexpr int kReasonWords = 9 + 1024 + 8 + 5;   // msspe_ctx::d_reasons (int_core.hpp IntArgs::reasons); the last five: pairs
constexpr int kBoundSurvivors = kReasonWords - 5;   // the bound first stage handed on, and its probe launch's count;
constexpr int kBoundListStats = kReasonWords - 3;   // the bound list stage: entries of list U, ordered pairs it appended;
constexpr int kBoundWindowSurvivors = kReasonWords - 1;   // ordered pairs the windowed first stage sent to list U as not culled
constexpr int kOvfCounters = 9;                     // msspe_ctx::ovf_count: the eight stage counters, then list U's
constexpr int kOvfU = 8;
constexpr long kBoundProbePairs = 1L << 20;  // pair_bound = auto: pairs of the probe launch behind a new record
// pair_bound = auto runs the bound stage while the recorded survivor share is at most this: HALF the break-even share
//   (ns per pair of the exact row kernel - ns per pair of the bound kernel) / ns per handed-on pair of the list chain
// = (0.2856 - 0.1521) / 1.72 = 7.8 % (DESIGN.md 4.0 holds the three prices and the session they were measured in)
// (the mirrored stage of a square screen costs 0.0763 ns per ordered pair: its break-even share is about 15 %, so the
//  switch point stays on the safe side there)
constexpr float kBoundShareMax = 0.039f;
// pair_bound_window = auto: screens of at least this many pairs.  Below it -- the short chain's range (cross_dimer_impl) --
// a screen is a few launches whose time is latency, not the first stage's instruction count, and the longer list U only
// adds to the flush
constexpr long kWindowAutoMinPairs = 1L << 23;

}  // namespace

// Engine options (msspe_set_option): which kernels a call may use.  Defaults are the product path;
// the rest exists for the parity tests (every stage against every other) and for experiments.
struct EngineOptions {
    int pair_kernel = 0;      // 0 auto | 1 f64 register-table kernel first | 2 general integer kernel first
    bool force_generic = false;
    int split_min_k = 16;     // 14- and 15-mers: the row-specialised first stage (round 3); 16 and up: the split-table kernel
    bool wave_kernel = true;
    int list_cap_log2 = 0;    // 0: sized by the call; 20..30: fixed (forces flushes mid-screen)
    int split_lanes = 0;      // 0: by oligo length; 2 / 4 / 8
    bool row_oob = true;      // the row-specialised first stage (it reads LDS beyond its allocation: thal_pairs_row.hip) may run
    int pair_bound = 2;       // decision-only screens of up to 13 bases, cut <= 0: the bound first stage (k_pairs_bound) in front of
                              // the list stages -- 0 never | 1 wherever it applies | 2 auto: while few pairs survive it (kBoundShareMax)
    int pair_mirror = 2;      // the bound stage of a square same-pool screen fills each unordered pair once and hands a survivor on in
                              // both orders -- 0 never | 1, 2 (auto): wherever the tables are strand-symmetric (ChemEntry::mirror_ok)
    int pair_bound_list = 2;  // lanes that leave the bound first stage without a bound of their own go to list U and are bounded there
                              // (k_pairs_bound_list) before the exact lists -- 0 never | 1, 2 (auto): wherever the bound first stage runs
    int pair_bound_packed = 2;  // the bound first stage runs its packed instance (k_pairs_bound_packed: one register per slot, coarse
                              // units, 1,024 threads) -- 0 never | 1, 2 (auto): wherever the chemistry's range fits (ChemEntry::packed_ok)
    int pair_bound_window = 2;  // the packed first stage runs its WINDOWED instance (k_pairs_bound_window: a cell scans the rows of a
                              // window, one candidate stands for all rows above; what it does not cull goes to list U) -- 0 never |
                              // 1 wherever the packed instance would run, the chemistry's entry is usable (ChemEntry::window_ok) and
                              // pair_bound_list is on | 2 auto: the same, from kWindowAutoMinPairs pairs per screen
    int pair_bound_list_packed = 2;  // the bound list stage runs its packed instance (k_pairs_bound_list_packed: one register per
                              // slot, the packed first stage's units and cull rule, 1,024 threads) -- 0 never | 1 wherever the bound
                              // list stage runs behind the packed or the windowed first stage | 2 auto: the same, from
                              // kWindowAutoMinPairs pairs per screen
    bool split_list = true;   // short oligos: tables too large for the integer list stage go to the split kernel's list mode
    bool short_chain = true;  // screens of up to 2^23 pairs: integer list stage -> one wave per pair (no register-table stages between)
    int self_lane_from = 81920;   // oligos per call from which SELF_ANY / SELF_END run one lane per oligo (msspe_oligo_stats_dev)
    int site_list_cap_log2 = 22;  // msspe_background_thal*: work list of 2^this sites (44 bytes each: 185 MB)
    int amplicon_keys_cap_log2 = 20;  // msspe_background_amplicons*: the stable-key buffer starts at 2^this keys and doubles
    long panel_thin_matrix_max_mb = 8192;   // msspe_panel_thin*: the incidence matrix may take this much, else MSSPE_ERR_CAPACITY
    bool thin_thal_unique = true;   // msspe_panel_thin_thal*: a slab's matches are sorted and each distinct (primer, template) is scored once
    int conflict_graph_block_rows = 0;   // msspe_conflict_graph*: rows per block of the two per-rule planes (0: within kGraphPlaneBytes)
};

struct msspe_ctx {
    int device = 0;
    int n_cu = 256;
    bool lds_reads_zero = false;       // pairs_row_lds_reads_zero(): the row kernel may run
    EngineOptions opt;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    NNTables host_tb;
    NNTables *d_tb = nullptr;
    std::vector<ChemEntry> chem_cache;
    double *wsS = nullptr, *wsH = nullptr;
    size_t ws_cells = 0;
    uint2 *ovf_list = nullptr;         // pairs the main kernel could not hold
    uint2 *ovf_list2 = nullptr;        // pairs the wide kernel could not hold either
    uint32_t *ovf_count = nullptr;     // list counters of the stages (8): [0] first, [1] second, ...
    long list_cap = 0;                 // entries per hand-over list
    long list_cap_ceiling = 1L << 30;  // lowered when an allocation of that size failed (not tried again)
    uint64_t *d_ovf_total = nullptr;   // [0] pairs handed on so far, [1] != 0: a list counter went past its capacity,
                                       // [2 + q] pairs that entered list q (msspe_get_info "hand_over_list_<q>")
    unsigned long long *d_reasons = nullptr;   // [8] statistics of the integer stage
    uint64_t *d_sorted = nullptr;      // column primers grouped by composition
    uint32_t *d_perm = nullptr;
    void *d_sort_scratch = nullptr;    // keys, values and rocPRIM temporary storage of the composition sort
    size_t sort_cap = 0, sort_scratch_bytes = 0;
    uint64_t *d_ab = nullptr;          // msspe_cross_dimer_ab*: pool A and pool B staged back to back, A first
    size_t ab_cap = 0;
    std::string err;
    KmerStage kmer;
    KmerStage kmer_rev;                // direction 1 of msspe_kmer_candidates_both_packed_dev (its own buffers and loop graph)
    hipStream_t stream_rev = nullptr;  // ... and its stream
    hipEvent_t ev_rev = nullptr;
    MismatchCoverage mm_cov;           // msspe_segment_coverage_mm*: primer words, counts, per-segment minima
    BackgroundSites background;        // msspe_background_sites*: primer words in plane form, per-primer counts
    CoverStage cover;                  // msspe_conflict_cover*: the symmetrised bitmap and the round state
    GraphScratch graph;                // msspe_conflict_graph*: the two per-rule planes of a row block, its row counts and bases
    TubeStage tubes;                   // msspe_conflict_tubes*: its round state (the graph lives in cover's buffers)
    PanelThin thin;                    // msspe_panel_thin*: the incidence matrix, covered words, gains and round state
    PanelThinThal thin_thal;           // msspe_panel_thin_thal*: the sorted order, run slots and rocPRIM storage of a slab (its
                                       // matrix and round state are thin's, its work list site_work, its plane words cov_thal's)
    PanelSelect select;                // msspe_panel_select*: its pool, masks, gains and round state (the graph lives in
                                       // cover's buffers, the matrix in thin's)
    hipEvent_t select_ev[2] = {};      // ... around its incidence pass
    long long select_prepare_us = 0, select_incidence_us = 0;
    CoverageThal cov_thal;             // msspe_segment_coverage_thal*: plane words, per-segment words, cell bitmaps,
                                       // counters, the caller's list (its work list is site_work below)
    // msspe_background_thal*: the work list (site records, their pairs, raw dG and t), the site pool [primers | site
    // oligos], 4 n counts (sites, then stable sites) and the slab's site counter; with a template flank also the
    // sites' class codes, and the class counters with the grouping cursors behind them
    struct SiteWork {
        msspe_site *sites = nullptr;
        uint2 *list = nullptr;
        double *dg = nullptr, *t = nullptr;
        size_t cap = 0;
        uint64_t *pool = nullptr;
        size_t pool_cap = 0;
        unsigned long long *counts = nullptr;
        size_t counts_cap = 0;
        uint64_t *slab_count = nullptr;
        uint8_t *cls = nullptr;
        size_t cls_cap = 0;
        uint32_t *class_counts = nullptr;   // [kSiteClasses] sites per class, [kSiteClasses] cursors
        long long slabs = 0, redone = 0;   // of the last call
        long long flank_classes = 0, truncated = 0;
    } site_work;
    // msspe_background_amplicons*: the stable keys as the fold appends them (grown by doubling) and their count, the
    // sorted keys with their record ids, rocPRIM's temporary storage, the record starts, 2 n amplicon counts
    struct AmpWork {
        uint64_t *keys = nullptr;
        size_t keys_cap = 0;
        uint64_t *key_count = nullptr;
        uint64_t *sorted = nullptr;
        uint32_t *rec = nullptr;
        size_t sorted_cap = 0;
        void *tmp = nullptr;
        size_t tmp_bytes = 0;
        uint64_t *starts = nullptr;
        size_t starts_cap = 0;
        unsigned long long *counts = nullptr;
        size_t counts_cap = 0;
        hipEvent_t ev[3] = {};             // before the sort, between record ids and join, after the join
        long long n_keys = 0, grows = 0;   // of the last call
        long long sort_us = 0, join_us = 0;
    } amp_work;
    // msspe_stream_reach*: the three bit planes (plus sites, minus sites, reached by neither) in one allocation, the
    // three tile arrays in another, the record starts and the per-record sums
    struct ReachWork {
        uint64_t *planes = nullptr;
        size_t plane_words = 0;            // capacity of one plane, in words
        uint32_t *tiles = nullptr;
        size_t tiles_cap = 0;              // capacity of one tile array
        uint64_t *starts = nullptr;
        ReachAccum *acc = nullptr;
        size_t records_cap = 0;
        hipEvent_t ev[7] = {};             // around the six launches behind the scored pass
        long long grows = 0;               // of the last call
        long long us[6] = {};              // tiles, scan, masks, gap tiles, scan, gaps
    } reach_work;
    PanelThinReach thin_reach;         // msspe_panel_thin_reach*: the intervals, ranks, gains and round state (the keys are
                                       // amp_work's, the planes and record starts reach_work's)
    // optional profiling of the dominant kernel (k_pairs_fast) with HIP events on ctx->stream
    bool prof_on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
    long long bound_mirrored = 0;      // info key "bound_mirrored"
    // msspe_kmer_candidates_tolerant*: the seeding passes of a call (one per direction) take turns on the context's
    // stream, matrix and work list; of the last call, both directions added up
    struct Tolerant {
        std::mutex turn;
        hipEvent_t ev[3] = {};             // before the incidence, between it and the seeding, after the seeding
        long long tiles = 0, segments = 0, incidence_us = 0, seed_us = 0;
    } tolerant;
};

namespace {

int fail(msspe_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

int hip_fail(msspe_ctx *ctx, hipError_t e, const char *what)
{
    return fail(ctx, MSSPE_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(ctx, expr)                                              \
    do {                                                                \
        hipError_t e__ = (expr);                                        \
        if (e__ != hipSuccess) return hip_fail((ctx), e__, #expr);      \
    } while (0)

std::string default_bundle_path()
{
    Dl_info info;
    if (dladdr((void *)&msspe_version, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        const size_t slash = p.find_last_of('/');
        p = slash == std::string::npos ? std::string(".") : p.substr(0, slash);
        return p + "/data/nn_params.bundle";
    }
    return "data/nn_params.bundle";
}

bool same_chem(const msspe_chem &a, const msspe_chem &b)
{
    return a.mv == b.mv && a.dv == b.dv && a.dntp == b.dntp && a.dna_conc == b.dna_conc &&
           a.temp_c == b.temp_c && a.max_loop == b.max_loop;
}

// Which kernels may answer a pair under these tables (ChemEntry's flags), with the device tables they go with:
// chem_entry() and msspe_host_table_routes() both decide here and nowhere else.
struct TableRoutes {
    bool fast_ok = false, int_ok = false, row_ok = false;
    int split_max_k = 0, wave_max_k = 0;
};

TableRoutes table_routes(const NNTables &tb, const PairTables &pt, int max_loop, FastTables &ft, IntTables &it,
                         SplitTables &st)
{
    TableRoutes r;
    r.fast_ok = build_fast_tables(tb, pt, pairs_fast_max_k(), ft);
    r.int_ok = r.fast_ok && build_int_tables(ft, pairs_fast_max_k(), it);
    r.row_ok = r.int_ok && pairs_row_tables_ok(it);
    r.split_max_k = build_split_tables(pt, max_loop, st) ? st.max_k : 0;
    r.wave_max_k = st.f64_max_k;
    return r;
}

// kind: kCutEndT is the entry of the END screen (msspe_cross_dimer_end*), whose cut is msspe_t_cut(threshold), and
// kCutAnyT that of an ANY fill decided on t (msspe_background_thal*, mode 1); each kind is cached apart from the
// others of the same chemistry and threshold, so that no call can pick up another's cut.
int chem_entry(msspe_ctx *ctx, const msspe_chem &chem, float threshold, ChemEntry **out, int kind = kCutAnyDg)
{
    for (auto &e : ctx->chem_cache)
        if (same_chem(e.chem, chem) && e.kind == kind && (e.threshold == threshold ||
                                        (std::isnan(e.threshold) && std::isnan(threshold)))) {
            *out = &e;
            return MSSPE_OK;
        }
    if (!(chem.dna_conc > 0) || chem.max_loop < 0 || chem.max_loop > 30)
        return fail(ctx, MSSPE_ERR_ARG, "chemistry: dna_conc must be > 0 and 0 <= max_loop <= 30");
    ChemEntry e;
    e.chem = chem;
    e.threshold = threshold;
    e.kind = kind;
    PairTables host_pt[2];
    for (int sym = 0; sym < 2; ++sym) {
        e.c[sym] = make_dimer_consts(chem.mv, chem.dv, chem.dntp, chem.dna_conc, chem.temp_c,
                                     chem.max_loop, sym == 1, threshold);
        std::string err;
        if (!build_pair_tables(ctx->host_tb, e.c[sym], host_pt[sym], err))
            return fail(ctx, MSSPE_ERR_TABLES, err);
    }
    HIP_TRY(ctx, hipMalloc((void **)&e.d_pt, sizeof host_pt));
    HIP_TRY(ctx, hipMemcpy(e.d_pt, host_pt, sizeof host_pt, hipMemcpyHostToDevice));
    {
        auto ft = std::make_unique<FastTables>();
        auto it = std::make_unique<IntTables>();
        auto st = std::make_unique<SplitTables>();
        const TableRoutes r = table_routes(ctx->host_tb, host_pt[0], chem.max_loop, *ft, *it, *st);
        e.fast_ok = r.fast_ok;
        e.int_ok = r.int_ok;
        e.row_ok = r.row_ok;
        e.split_max_k = r.split_max_k;
        e.wave_max_k = r.wave_max_k;
        HIP_TRY(ctx, hipMalloc((void **)&e.d_ft, sizeof(FastTables)));
        HIP_TRY(ctx, hipMemcpy(e.d_ft, ft.get(), sizeof(FastTables), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMalloc((void **)&e.d_it, sizeof(IntTables)));
        HIP_TRY(ctx, hipMemcpy(e.d_it, it.get(), sizeof(IntTables), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMalloc((void **)&e.d_st, sizeof(SplitTables)));
        HIP_TRY(ctx, hipMemcpy(e.d_st, st.get(), sizeof(SplitTables), hipMemcpyHostToDevice));
        if (kind == kCutAnyDg && r.row_ok) {
            auto bt = std::make_unique<BoundTables>();
            e.bound_ok = build_bound_tables(*ft, e.c[0], pairs_bound_max_k(), *bt);
            e.mirror_ok = e.bound_ok && bt->mirror_ok != 0;
            if (e.bound_ok) {
                HIP_TRY(ctx, hipMalloc((void **)&e.d_bt, sizeof(BoundTables)));
                HIP_TRY(ctx, hipMemcpy(e.d_bt, bt.get(), sizeof(BoundTables), hipMemcpyHostToDevice));
                auto bp = std::make_unique<BoundPacked>();
                e.packed_ok = build_bound_packed(*bt, pairs_bound_max_k(), *bp);
                if (e.packed_ok) {
                    e.packed_shift = bp->shift;
                    e.packed_bias = bp->bias;
                    HIP_TRY(ctx, hipMalloc((void **)&e.d_btq, sizeof(BoundTables)));
                    HIP_TRY(ctx, hipMemcpy(e.d_btq, &bp->q, sizeof(BoundTables), hipMemcpyHostToDevice));
                    e.window_ok = build_bound_window(*bp, pairs_bound_window_rows(), e.window);
                }
            }
        }
    }
    if (kind != kCutAnyDg)
        for (auto &c : e.c) c.g_cut = t_cut(threshold);
    ctx->chem_cache.push_back(e);
    *out = &ctx->chem_cache.back();
    return MSSPE_OK;
}

int ensure_workspace(msspe_ctx *ctx, size_t cells_per_lane)
{
    if (ctx->ws_cells >= cells_per_lane) return MSSPE_OK;
    if (ctx->wsS) (void)hipFree(ctx->wsS);
    if (ctx->wsH) (void)hipFree(ctx->wsH);
    ctx->wsS = ctx->wsH = nullptr;
    ctx->ws_cells = 0;
    const size_t bytes = cells_per_lane * kGenericLanes * sizeof(double);
    HIP_TRY(ctx, hipMalloc((void **)&ctx->wsS, bytes));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->wsH, bytes));
    ctx->ws_cells = cells_per_lane;
    return MSSPE_OK;
}

// The lists are sized by the call (every pair could be handed on between two flushes): small
// screens keep small lists, the 65,536-primer screen flushes every 8 launches.
int ensure_overflow(msspe_ctx *ctx, long total_pairs)
{
    // the small counter buffers first and unconditionally: a failed list allocation must not leave a
    // context whose counters are missing
    if (!ctx->ovf_count) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->ovf_count, sizeof(uint32_t) * kOvfCounters));
        HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, sizeof(uint32_t) * kOvfCounters, ctx->stream));
    }
    if (!ctx->d_ovf_total) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_ovf_total, kOvfTotals * sizeof(uint64_t)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_ovf_total, 0, kOvfTotals * sizeof(uint64_t), ctx->stream));
    }
    if (!ctx->d_reasons) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_reasons, kReasonWords * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_reasons, 0, kReasonWords * sizeof(unsigned long long), ctx->stream));
    }
    long want = kListCapMin;
    while (want < total_pairs && want < kListCapMax && want < ctx->list_cap_ceiling) want <<= 1;
    const bool fixed = ctx->opt.list_cap_log2 >= 20 && ctx->opt.list_cap_log2 <= 30;
    if (fixed) want = 1L << ctx->opt.list_cap_log2;
    if (ctx->ovf_list && ctx->ovf_list2 && (ctx->list_cap == want || (ctx->list_cap > want && !fixed))) return MSSPE_OK;
    if (ctx->ovf_list || ctx->ovf_list2) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->ovf_list) (void)hipFree(ctx->ovf_list);
        if (ctx->ovf_list2) (void)hipFree(ctx->ovf_list2);
        ctx->ovf_list = ctx->ovf_list2 = nullptr;
        ctx->list_cap = 0;
    }
    // The large sizes only buy fewer flushes: when the card is short of memory (the caller's own tensors), a
    // smaller pair of lists does, down to what one launch can fill.
    const long floor_cap = std::max(kListCapMin, std::min(want, kChunkPairs));
    for (;;) {
        hipError_t e1 = hipMalloc((void **)&ctx->ovf_list, sizeof(uint2) * (size_t)want);
        hipError_t e2 = e1 == hipSuccess ? hipMalloc((void **)&ctx->ovf_list2, sizeof(uint2) * (size_t)want) : e1;
        if (e1 == hipSuccess && e2 == hipSuccess) break;
        // all or nothing: a later call starts from a clean state
        if (ctx->ovf_list) (void)hipFree(ctx->ovf_list);
        if (ctx->ovf_list2) (void)hipFree(ctx->ovf_list2);
        ctx->ovf_list = ctx->ovf_list2 = nullptr;
        ctx->list_cap = 0;
        (void)hipGetLastError();
        if (fixed || want <= floor_cap) return hip_fail(ctx, e1 != hipSuccess ? e1 : e2, "hipMalloc(hand-over lists)");
        want >>= 1;
        ctx->list_cap_ceiling = want;
    }
    ctx->list_cap = want;
    return MSSPE_OK;
}

int ensure_sort(msspe_ctx *ctx, size_t ncols)
{
    if (ctx->sort_cap >= ncols) return MSSPE_OK;
    if (ctx->d_sorted) (void)hipFree(ctx->d_sorted);
    if (ctx->d_perm) (void)hipFree(ctx->d_perm);
    if (ctx->d_sort_scratch) (void)hipFree(ctx->d_sort_scratch);
    ctx->d_sorted = nullptr;
    ctx->d_perm = nullptr;
    ctx->d_sort_scratch = nullptr;
    ctx->sort_cap = 0;
    ctx->sort_scratch_bytes = pool_sort_scratch_bytes(ncols);
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sorted, sizeof(uint64_t) * ncols));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_perm, sizeof(uint32_t) * ncols));
    HIP_TRY(ctx, hipMalloc(&ctx->d_sort_scratch, ctx->sort_scratch_bytes));
    ctx->sort_cap = ncols;
    return MSSPE_OK;
}

// End of a flush: totals for the statistics (all pairs the first stage handed on, and per list the pairs that
// entered it), and the check that no stage's list counter went past the capacity of its list (entries beyond it
// are not stored: the host sizes the flushes so that this cannot happen, and a screen during which it did must not
// be trusted).
__global__ void k_accumulate_overflow(const uint32_t *count, uint64_t *total, uint32_t cap)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        total[0] += count[0];
        for (int q = 0; q < 7; ++q) {
            total[2 + q] += count[q];
            if (count[q] > cap) total[1] = 1;
        }
        if (count[kOvfU] > cap) total[1] = 1;   // list U (the bound list stage's input): checked, not part of the totals
    }
}

// A device allocation that is freed when it goes out of scope (move-only): the host-buffer entry points return
// from any failed step without a cleanup list.
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc((void **)&p, sizeof(T) * count); }
    operator T *() const { return p; }
};

// "Pack one pool or fail with the K / ACGT message" and "pack A and B back to back, A first" of the ASCII wrappers.
int pack_pool(msspe_ctx *ctx, const char *ascii, int n, int k, std::vector<uint64_t> &packed)
{
    packed.resize((size_t)n);
    const int rc = msspe_pack_oligos(ascii, n, k, packed.data());
    if (rc) return fail(ctx, rc, rc == MSSPE_ERR_K ? "oligo length must be 1..32"
                                                   : "pool holds characters other than ACGT");
    return MSSPE_OK;
}

int pack_ab(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b, int k_b,
            std::vector<uint64_t> &packed)
{
    if (k_a < 2 || k_a > 32 || k_b < 2 || k_b > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if ((long)n_a + (long)n_b > (long)INT32_MAX) return fail(ctx, MSSPE_ERR_ARG, "pools too large");
    packed.resize((size_t)n_a + (size_t)n_b);
    if (msspe_pack_oligos(a_ascii ? a_ascii : "", n_a, k_a, packed.data()) ||
        msspe_pack_oligos(b_ascii ? b_ascii : "", n_b, k_b, packed.data() + n_a))
        return fail(ctx, MSSPE_ERR_ARG, "pool holds characters other than ACGT");
    return MSSPE_OK;
}

// One block of a screen: rows [row0, row1) of k bases against columns [col0, col1) of k2 bases (k2 != k: the
// rectangular chain) of one pool of n oligos, and where the results go.  Filled once, where a public entry point
// receives its arguments; the host-buffer wrappers receive one whose pool is still to be uploaded and whose sinks
// are host pointers, and mirror it on the device.
struct ScreenBlock {
    const uint64_t *pool;
    int n, k, k2;
    int row0, row1, col0, col1;
    PairSinks sinks;   // row0 / col0 / ncols / words follow the block's ranges
};

PairSinks plane_sinks(uint32_t *row_conflicts, uint64_t *bitmap, double *dg, double *tm)
{
    PairSinks s;
    std::memset(&s, 0, sizeof s);
    s.row_conflicts = row_conflicts;
    s.bitmap = bitmap;
    s.dg = dg;
    s.tm = tm;
    return s;
}

// edges: msspe_edge_dev / msspe_end_edge_dev records (the layout of EdgeRecord)
PairSinks edge_sinks(uint32_t *row_conflicts, void *edges, uint64_t *count, uint64_t capacity)
{
    static_assert(sizeof(msspe_edge_dev) == sizeof(EdgeRecord) && sizeof(msspe_end_edge_dev) == sizeof(EdgeRecord),
                  "edge record layouts differ");
    PairSinks s = plane_sinks(row_conflicts, nullptr, nullptr, nullptr);
    s.edges = static_cast<EdgeRecord *>(edges);
    s.edge_count = reinterpret_cast<unsigned long long *>(count);
    s.edge_cap = capacity;
    return s;
}

ScreenBlock screen_block(const uint64_t *pool, int n, int k, int k2, int row0, int row1, int col0, int col1,
                         const PairSinks &sinks)
{
    ScreenBlock b{pool, n, k, k2, row0, row1, col0, col1, sinks};
    b.sinks.row0 = row0;
    b.sinks.col0 = col0;
    b.sinks.ncols = col1 - col0;
    b.sinks.words = (b.sinks.ncols + 63) / 64;
    return b;
}

// May the register-table kernels (thal_pairs.hip: no loop-size cut-off) take oligos of k bases under this chemistry?
bool reg_tables_ok(const msspe_ctx *ctx, const ChemEntry *ce, int k)
{
    return !ctx->opt.force_generic && k <= pairs_fast_max_k() && ce->fast_ok && ce->chem.max_loop >= 2 * k - 4;
}

// May the wave kernel (f64, one wave per pair) take pairs whose longer oligo has kmax bases?
bool wave_ok(const msspe_ctx *ctx, const ChemEntry *ce, int kmax)
{
    return !ctx->opt.force_generic && kmax <= ce->wave_max_k && ctx->opt.wave_kernel;
}

// The pair kernels' arguments for the block in list mode; first_stage_args puts a launch on top.
PairKernelArgs pair_args(const msspe_ctx *ctx, const ChemEntry *ce, const ScreenBlock &b)
{
    PairKernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.ft = ce->d_ft;
    a.c = ce->c[0];
    a.pool = b.pool;
    a.n = b.n;
    a.k = b.k;
    a.k2 = b.k2;
    a.row0 = b.row0;
    a.row1 = b.row1;
    a.col1 = b.col1 - b.col0;
    a.sinks = b.sinks;
    a.work_counter = ctx->ovf_count + 7;   // the last of the eight stage counters
    return a;
}

// ... for one first-stage launch: its rows and columns (screen_plan.hpp: sorted positions, the wave kernel's are pool
// columns), the composition-sorted columns (ensure_sort) and hand-over list 0 (ensure_overflow) with its capacity.
PairKernelArgs first_stage_args(const msspe_ctx *ctx, const ChemEntry *ce, const ScreenBlock &b, const Launch &l)
{
    PairKernelArgs a = pair_args(ctx, ce, b);
    a.cols_sorted = ctx->d_sorted;
    a.perm = ctx->d_perm;
    a.ncols_sorted = b.sinks.ncols;
    a.row0 = l.row0;
    a.row1 = l.row1;
    a.col0 = l.col0;
    a.col1 = l.col1;
    a.overflow_list = ctx->ovf_list;
    a.overflow_count = ctx->ovf_count;
    a.overflow_cap = (uint32_t)ctx->list_cap;
    return a;
}

// The dense kernel's arguments for the block; the caller sets its work (list / n_work, self_mode, detail).
GenericDimerArgs dimer_args(const msspe_ctx *ctx, const ChemEntry *ce, const ScreenBlock &b, int mode)
{
    GenericDimerArgs g;
    std::memset(&g, 0, sizeof g);
    g.pt = ce->d_pt;
    g.c[0] = ce->c[0];
    g.c[1] = ce->c[1];
    g.pool = b.pool;
    g.k = b.k;
    g.k2 = b.k2;
    g.mode = mode;
    g.sinks = b.sinks;
    g.wsS = ctx->wsS;
    g.wsH = ctx->wsH;
    g.ws_lanes = kGenericLanes;
    return g;
}

// The stages that may stand behind a first stage, each over the hand-over list the stage before it wrote.  A route
// (StageList) names them in the order they run and ends with Dense, which takes whatever is left.  The order of a
// route is written where the route is chosen -- cross_dimer_impl (ANY), cross_dimer_end_impl (END),
// score_site_pairs (an explicit list) -- and nowhere else; include/msspe_hip.h ("hand_over_list_<q>") documents
// the result: the stage at position q of a route reads list q.
enum class ListStage {
    IntList,     // the integer kernel again, 64 slots, lanes sorted by table size: pairs that only left their wave
                 // because of their size (marked entries -- exact ties -- pass through to the f64 stages)
    SplitList,   // tables beyond the integer list stage's 63 stored cells: two lanes per pair, still exact integers
    MainList,    // the 56-slot f64 register table: exact ties
    Wide,        // the 72-slot f64 register table
    Wave,        // huge tables: f64, one wave per pair, the table in LDS
    Dense        // last: both-self-complementary pairs, tables beyond the wave kernel's
};

struct StageList {
    ListStage at[6];
    int n = 0;
    void add(ListStage s) { at[n++] = s; }
};

// The hand-over lists behind a first stage.  A list stage reads the current list (counter q) and appends what it
// does not answer to the next (counter q + 1); the first list is the context's ovf_list (what a first stage wrote)
// or a caller's own, and behind it the context's two buffers ping-pong: a stage's input is consumed when it ends.
struct ListChain {
    msspe_ctx *ctx;
    const ChemEntry *ce;
    bool end1;             // the END1 instantiations of the f64 stages
    const uint2 *in_list;
    uint32_t *in_count;
    long in_work;          // most entries the current list can hold: first_work on the first list, then the capacity
    uint2 *out_list;
    uint32_t *out_count;
    long cap;              // entries per hand-over list

    ListChain(msspe_ctx *ctx_, const ChemEntry *ce_, bool end1_, const uint2 *first_list, long first_work)
        : ctx(ctx_), ce(ce_), end1(end1_), in_list(first_list), in_count(ctx_->ovf_count), in_work(first_work),
          out_list(first_list == ctx_->ovf_list ? ctx_->ovf_list2 : ctx_->ovf_list), out_count(ctx_->ovf_count + 1),
          cap(ctx_->list_cap)
    {
    }

    int stage(ListStage s, PairKernelArgs &a)
    {
        a.overflow_list = out_list;
        a.overflow_count = out_count;
        a.overflow_cap = (uint32_t)cap;
        switch (s) {
        case ListStage::IntList:
            HIP_TRY(ctx, launch_pairs_int_list(a, ce->d_it, in_list, in_count, ctx->d_reasons, ctx->n_cu, ctx->stream,
                                           ce->row_ok));
            break;
        case ListStage::SplitList:
            HIP_TRY(ctx, launch_pairs_split_list(a, ce->d_st, in_list, in_count, ctx->n_cu, ctx->stream));
            break;
        case ListStage::MainList: HIP_TRY(ctx, launch_pairs_main_list(a, in_list, in_count, ctx->stream, end1)); break;
        case ListStage::Wide: HIP_TRY(ctx, launch_pairs_wide(a, in_list, in_count, ctx->stream, end1)); break;
        case ListStage::Wave: HIP_TRY(ctx, launch_pairs_wave(a, ce->d_st, in_list, in_count, ctx->stream, end1)); break;
        case ListStage::Dense: return fail(ctx, MSSPE_ERR_ARG, "the dense kernel ends a route: ListChain::finish");
        }
        in_list = out_list;
        in_count = out_count;
        in_work = cap;
        out_list = out_list == ctx->ovf_list ? ctx->ovf_list2 : ctx->ovf_list;
        ++out_count;
        return MSSPE_OK;
    }

    // The dense kernel over the current list; accumulate: the totals of the hand-over statistics and the overrun
    // check (k_accumulate_overflow); then the eight counters and list U's are cleared for the next flush or call.
    int finish(GenericDimerArgs &g, bool accumulate)
    {
        g.list = in_list;
        g.list_count = in_count;
        g.n_work = in_work;
        HIP_TRY(ctx, launch_dimer_generic(g, ctx->stream, end1));
        if (accumulate)
            hipLaunchKernelGGL(k_accumulate_overflow, dim3(1), dim3(64), 0, ctx->stream, ctx->ovf_count,
                               ctx->d_ovf_total, (uint32_t)cap);
        HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, kOvfCounters * sizeof(uint32_t), ctx->stream));
        return MSSPE_OK;
    }

    int run(const StageList &route, PairKernelArgs &a, GenericDimerArgs &g, bool accumulate)
    {
        for (int q = 0; q < route.n && route.at[q] != ListStage::Dense; ++q)
            if (int rc = stage(route.at[q], a)) return rc;
        return finish(g, accumulate);
    }
};

}  // namespace

namespace msspe {
hipStream_t ctx_stream(msspe_ctx *ctx) { return ctx->stream; }   // group.hip: collectives are enqueued on the members' streams
}

extern "C" {

const char *msspe_version(void) { return "msspe-hip 0.1.0 (gfx950)"; }

void msspe_chem_ntthal_defaults(msspe_chem *c)
{
    if (!c) return;
    c->mv = 50.0;
    c->dv = 3.0;
    c->dntp = 0.0;
    c->dna_conc = 250.0;
    c->temp_c = 25.0;
    c->max_loop = 30;
}

void msspe_chem_primer3_defaults(msspe_chem *c)
{
    if (!c) return;
    c->mv = 50.0;
    c->dv = 1.5;
    c->dntp = 0.6;
    c->dna_conc = 50.0;
    c->temp_c = 37.0;
    c->max_loop = 30;
}

int msspe_create(int device, const char *params_path, msspe_ctx **out)
{
    if (!out) return MSSPE_ERR_ARG;
    *out = nullptr;
    msspe_ctx *ctx = new (std::nothrow) msspe_ctx();
    if (!ctx) return MSSPE_ERR_NOMEM;
    *out = ctx;   // returned even on failure so that msspe_last_error() works; destroy it anyway
    ctx->device = device;
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, ctx->host_tb, err)) return fail(ctx, MSSPE_ERR_TABLES, err);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(ctx, MSSPE_ERR_DEVICE,
                    "no HIP device available: this engine has no CPU fallback (needs gfx950)");
    if (device < 0 || device >= ndev) return fail(ctx, MSSPE_ERR_ARG, "device ordinal out of range");
    HIP_TRY(ctx, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ctx, MSSPE_ERR_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_tb, sizeof(NNTables)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_tb, &ctx->host_tb, sizeof(NNTables), hipMemcpyHostToDevice));
    // the row-specialised kernel drops its address clamp where LDS reads beyond the allocation return 0
    // (thal_pairs_row.hip kRowZero): every gfx950 seen does; a device that does not, and a context with option
    // row_oob = 0 (debugger sessions that trap on out-of-range LDS accesses), runs the general integer kernel
    HIP_TRY(ctx, pairs_row_lds_reads_zero(ctx->stream, ctx->n_cu, &ctx->lds_reads_zero));
    return MSSPE_OK;
}

int msspe_set_option(msspe_ctx *ctx, const char *key, const char *value)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!key || !value) return fail(ctx, MSSPE_ERR_ARG, "msspe_set_option: null key or value");
    const std::string k(key), v(value);
    char *end = nullptr;
    const long num = std::strtol(value, &end, 10);
    const bool is_num = end && end != value && *end == '\0';
    auto bad = [&]() { return fail(ctx, MSSPE_ERR_ARG, "msspe_set_option: bad value '" + v + "' for '" + k + "'"); };
    if (k == "pair_kernel") {
        if (v == "auto") ctx->opt.pair_kernel = 0;
        else if (v == "f64") ctx->opt.pair_kernel = 1;
        else if (v == "int") ctx->opt.pair_kernel = 2;
        else return bad();
    } else if (k == "force_generic") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.force_generic = num != 0;
    } else if (k == "split_min_k") {
        if (!is_num || num < 2 || num > 99) return bad();
        ctx->opt.split_min_k = (int)num;
    } else if (k == "wave_kernel") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.wave_kernel = num != 0;
    } else if (k == "list_cap_log2") {
        if (!is_num || !(num == 0 || (num >= 20 && num <= 30))) return bad();
        ctx->opt.list_cap_log2 = (int)num;
    } else if (k == "split_lanes") {
        if (!is_num || !(num == 0 || num == 2 || num == 4 || num == 8)) return bad();
        ctx->opt.split_lanes = (int)num;
    } else if (k == "split_list") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.split_list = num != 0;
    } else if (k == "short_chain") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.short_chain = num != 0;
    } else if (k == "self_lane_from") {
        if (!is_num || num < 0) return bad();
        ctx->opt.self_lane_from = (int)num;
    } else if (k == "site_list_cap_log2") {
        if (!is_num || num < 12 || num > 26) return bad();   // 2^12: what one run against one primer can hold
        ctx->opt.site_list_cap_log2 = (int)num;
    } else if (k == "amplicon_keys_cap_log2") {
        if (!is_num || num < 10 || num > 28) return bad();
        ctx->opt.amplicon_keys_cap_log2 = (int)num;
    } else if (k == "panel_thin_matrix_max_mb") {
        if (!is_num || num < 1 || num > (1L << 20)) return bad();
        ctx->opt.panel_thin_matrix_max_mb = num;
    } else if (k == "thin_thal_unique") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.thin_thal_unique = num != 0;
    } else if (k == "conflict_graph_block_rows") {
        if (!is_num || num < 0 || num > (long)INT32_MAX) return bad();
        ctx->opt.conflict_graph_block_rows = (int)num;
    } else if (k == "row_oob") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->opt.row_oob = num != 0;
    } else if (k == "pair_bound") {
        if (v == "auto") ctx->opt.pair_bound = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_bound = (int)num;
        else return bad();
    } else if (k == "pair_mirror") {
        if (v == "auto") ctx->opt.pair_mirror = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_mirror = (int)num;
        else return bad();
    } else if (k == "pair_bound_window") {
        if (v == "auto") ctx->opt.pair_bound_window = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_bound_window = (int)num;
        else return fail(ctx, MSSPE_ERR_ARG, "pair_bound_window: 0, 1 or auto");
    } else if (k == "pair_bound_packed") {
        if (v == "auto") ctx->opt.pair_bound_packed = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_bound_packed = (int)num;
        else return bad();
    } else if (k == "pair_bound_list_packed") {
        if (v == "auto") ctx->opt.pair_bound_list_packed = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_bound_list_packed = (int)num;
        else return bad();
    } else if (k == "pair_bound_list") {
        if (v == "auto") ctx->opt.pair_bound_list = 2;
        else if (is_num && (num == 0 || num == 1)) ctx->opt.pair_bound_list = (int)num;
        else return bad();
    } else if (k == "stage_a_graph") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->kmer.set_use_graph(num != 0);
        ctx->kmer_rev.set_use_graph(num != 0);
    } else if (k == "stage_a_candidates") {
        if (!is_num || num < 0 || num > 1) return bad();
        ctx->kmer.set_narrow_loop(num != 0);
        ctx->kmer_rev.set_narrow_loop(num != 0);
    } else {
        return fail(ctx, MSSPE_ERR_ARG, "msspe_set_option: unknown option '" + k + "'");
    }
    return MSSPE_OK;
}

int msspe_get_info(msspe_ctx *ctx, const char *key, long long *value_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!key || !value_out) return fail(ctx, MSSPE_ERR_ARG, "msspe_get_info: null key or output");
    const std::string k(key);
    if (k == "device") *value_out = ctx->device;
    else if (k == "n_cu") *value_out = ctx->n_cu;
    else if (k == "lds_reads_zero") *value_out = ctx->lds_reads_zero ? 1 : 0;
    else if (k == "row_kernel") {
        // ... and with the tables of every chemistry used so far (ChemEntry::row_ok)
        bool tables_ok = true;
        for (const auto &e : ctx->chem_cache) tables_ok = tables_ok && e.row_ok;
        *value_out = ctx->lds_reads_zero && ctx->opt.row_oob && ctx->opt.pair_kernel == 0 && !ctx->opt.force_generic &&
                     tables_ok ? 1 : 0;
    }
    else if (k == "stage_a_fast_iterations") *value_out = ctx->kmer.loop_stats()[0];
    else if (k == "stage_a_general_iterations") *value_out = ctx->kmer.loop_stats()[1];
    else if (k == "stage_a_rebuilds") *value_out = ctx->kmer.loop_stats()[2];
    else if (k == "stage_a_idle_iterations") *value_out = ctx->kmer.loop_stats()[3];
    else if (k == "site_list_cap_log2") *value_out = ctx->opt.site_list_cap_log2;
    else if (k == "background_thal_slabs") *value_out = ctx->site_work.slabs;
    else if (k == "background_thal_redone") *value_out = ctx->site_work.redone;
    else if (k == "background_thal_flank_classes") *value_out = ctx->site_work.flank_classes;
    else if (k == "background_thal_truncated") *value_out = ctx->site_work.truncated;
    else if (k == "coverage_thal_matches") *value_out = ctx->cov_thal.matches;
    else if (k == "coverage_thal_slabs") *value_out = ctx->cov_thal.slabs;
    else if (k == "coverage_thal_redone") *value_out = ctx->cov_thal.redone;
    else if (k == "coverage_thal_list_us") *value_out = ctx->cov_thal.list_us;
    else if (k == "coverage_thal_score_us") *value_out = ctx->cov_thal.score_us;
    else if (k == "coverage_thal_fold_us") *value_out = ctx->cov_thal.fold_us;
    else if (k == "amplicon_keys_cap_log2") *value_out = ctx->opt.amplicon_keys_cap_log2;
    else if (k == "amplicon_keys") *value_out = ctx->amp_work.n_keys;
    else if (k == "amplicon_key_grows") *value_out = ctx->amp_work.grows;
    else if (k == "amplicon_sort_us") *value_out = ctx->amp_work.sort_us;
    else if (k == "amplicon_join_us") *value_out = ctx->amp_work.join_us;
    else if (k == "reach_plane_bytes") *value_out = (long long)(3 * sizeof(uint64_t) * ctx->reach_work.plane_words);
    else if (k == "reach_grows") *value_out = ctx->reach_work.grows;
    else if (k == "reach_tile_columns") *value_out = kReachTileColumns;
    else if (k == "reach_tiles_us") *value_out = ctx->reach_work.us[0];
    else if (k == "reach_scan_us") *value_out = ctx->reach_work.us[1] + ctx->reach_work.us[4];
    else if (k == "reach_masks_us") *value_out = ctx->reach_work.us[2];
    else if (k == "reach_gap_tiles_us") *value_out = ctx->reach_work.us[3];
    else if (k == "reach_gaps_us") *value_out = ctx->reach_work.us[5];
    else if (k == "thin_reach_sites") *value_out = ctx->thin_reach.sites();
    else if (k == "thin_reach_intervals") *value_out = ctx->thin_reach.intervals();
    else if (k == "thin_reach_rounds") *value_out = ctx->thin_reach.rounds();
    else if (k == "thin_reach_prepare_us") *value_out = ctx->thin_reach.phase_us()[0];
    else if (k == "thin_reach_gain0_us") *value_out = ctx->thin_reach.phase_us()[1];
    else if (k == "thin_reach_rounds_us") *value_out = ctx->thin_reach.phase_us()[2];
    else if (k == "thin_reach_report_us") *value_out = ctx->thin_reach.phase_us()[3];
    else if (k == "cover_rounds") *value_out = ctx->cover.rounds();
    else if (k == "cover_keys_us") *value_out = ctx->cover.phase_us()[0];
    else if (k == "cover_symmetrise_us") *value_out = ctx->cover.phase_us()[1];
    else if (k == "cover_rounds_us") *value_out = ctx->cover.phase_us()[2];
    else if (k == "conflict_graph_grows") *value_out = ctx->graph.grows();
    else if (k == "tube_rounds") *value_out = ctx->tubes.rounds();
    else if (k == "tube_keys_us") *value_out = ctx->tubes.phase_us()[0];
    else if (k == "tube_symmetrise_us") *value_out = ctx->tubes.phase_us()[1];
    else if (k == "tube_rounds_us") *value_out = ctx->tubes.phase_us()[2];
    else if (k == "panel_thin_matrix_max_mb") *value_out = ctx->opt.panel_thin_matrix_max_mb;
    else if (k == "panel_thin_rounds") *value_out = ctx->thin.rounds();
    else if (k == "panel_thin_groups") *value_out = ctx->thin.groups();
    else if (k == "panel_thin_incidence_us") *value_out = ctx->thin.phase_us()[0];
    else if (k == "panel_thin_gain0_us") *value_out = ctx->thin.phase_us()[1];
    else if (k == "panel_thin_rounds_us") *value_out = ctx->thin.phase_us()[2];
    else if (k == "panel_thin_depth_shadows") *value_out = ctx->thin.depth_shadows();
    else if (k == "panel_thin_depth_colsum_us") *value_out = ctx->thin.depth_colsum_us();
    else if (k == "panel_select_rounds") *value_out = ctx->select.n_rounds();
    else if (k == "panel_select_tubes") *value_out = ctx->select.tubes_used();
    else if (k == "panel_select_barred") *value_out = ctx->select.barred();
    else if (k == "panel_select_prepare_us") *value_out = ctx->select_prepare_us;
    else if (k == "panel_select_incidence_us") *value_out = ctx->select_incidence_us;
    else if (k == "panel_select_rounds_us") *value_out = ctx->select.phase_us()[1];
    else if (k == "panel_select_first_us") *value_out = ctx->select.phase_us()[0];
    else if (k == "panel_select_depth_layers") *value_out = ctx->select.depth_layers();
    else if (k == "panel_select_depth_layer_us") *value_out = ctx->select.depth_layer_us();
    else if (k == "thin_thal_unique") *value_out = ctx->opt.thin_thal_unique ? 1 : 0;
    else if (k == "panel_thin_thal_matches") *value_out = ctx->thin_thal.matches;
    else if (k == "panel_thin_thal_unique_pairs") *value_out = ctx->thin_thal.unique_pairs;
    else if (k == "panel_thin_thal_slabs") *value_out = ctx->thin_thal.slabs;
    else if (k == "panel_thin_thal_redone") *value_out = ctx->thin_thal.redone;
    else if (k == "panel_thin_thal_list_us") *value_out = ctx->thin_thal.list_us;
    else if (k == "panel_thin_thal_unique_us") *value_out = ctx->thin_thal.unique_us;
    else if (k == "panel_thin_thal_score_us") *value_out = ctx->thin_thal.score_us;
    else if (k == "panel_thin_thal_fold_us") *value_out = ctx->thin_thal.fold_us;
    else if (k == "panel_thin_thal_rounds_us") *value_out = ctx->thin.phase_us()[2];
    else if (k == "stage_a_tolerant_tiles") *value_out = ctx->tolerant.tiles;
    else if (k == "stage_a_tolerant_segments") *value_out = ctx->tolerant.segments;
    else if (k == "stage_a_tolerant_incidence_us") *value_out = ctx->tolerant.incidence_us;
    else if (k == "stage_a_tolerant_seed_us") *value_out = ctx->tolerant.seed_us;
    else if (k == "pair_bound") *value_out = ctx->opt.pair_bound;
    else if (k == "pair_mirror") *value_out = ctx->opt.pair_mirror;
    else if (k == "pair_bound_list") *value_out = ctx->opt.pair_bound_list;
    else if (k == "pair_bound_packed") *value_out = ctx->opt.pair_bound_packed;
    else if (k == "pair_bound_list_packed") *value_out = ctx->opt.pair_bound_list_packed;
    else if (k == "pair_bound_window") *value_out = ctx->opt.pair_bound_window;
    else if (k == "bound_window_survivors") {
        // ordered pairs the windowed first stage could not cull and sent to list U since the last read of this key (reading
        // resets it).  bound_survivors counts what a first stage appended to list 0 as a survivor of ITS bound: the exact-unit
        // and packed instances do; the windowed one appends none -- behind it the bound list stage decides, and the pairs no
        // bound could cull are among bound_list_survivors
        *value_out = 0;
        if (!ctx->d_reasons) return MSSPE_OK;
        uint64_t v = 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(&v, ctx->d_reasons + kBoundWindowSurvivors, sizeof v, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_reasons + kBoundWindowSurvivors, 0, sizeof v, ctx->stream));
        *value_out = (long long)v;
    }
    else if (k == "bound_list_pairs" || k == "bound_list_survivors") {
        // the bound list stage since the last read of this key (reading resets it): entries of list U (unordered pairs under
        // the mirror), ordered pairs it appended to list 0
        *value_out = 0;
        if (!ctx->d_reasons) return MSSPE_OK;
        unsigned long long *at = ctx->d_reasons + kBoundListStats + (k == "bound_list_pairs" ? 0 : 1);
        uint64_t v = 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(&v, at, sizeof v, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemsetAsync(at, 0, sizeof v, ctx->stream));
        *value_out = (long long)v;
    }
    else if (k == "bound_mirrored") {
        // ordered pairs the mirrored bound stage answered or handed on without a fill of their own since the last read
        // of this key; reading resets it
        *value_out = ctx->bound_mirrored;
        ctx->bound_mirrored = 0;
    }
    else if (k == "bound_survivors") {
        // pairs the bound first stage handed on since the last read of this key; reading resets it
        *value_out = 0;
        if (!ctx->d_reasons) return MSSPE_OK;
        uint64_t v = 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(&v, ctx->d_reasons + kBoundSurvivors, sizeof v, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_reasons + kBoundSurvivors, 0, sizeof v, ctx->stream));
        *value_out = (long long)v;
    }
    else if (k.size() == 16 && k.compare(0, 15, "hand_over_list_") == 0 && k[15] >= '0' && k[15] <= '6') {
        // pairs that entered list q since the last read of this key; reading resets it
        *value_out = 0;
        if (!ctx->d_ovf_total) return MSSPE_OK;
        const size_t q = (size_t)(k[15] - '0');
        uint64_t v = 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(&v, ctx->d_ovf_total + 2 + q, sizeof v, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_ovf_total + 2 + q, 0, sizeof v, ctx->stream));
        *value_out = (long long)v;
    }
    else return fail(ctx, MSSPE_ERR_ARG, "msspe_get_info: unknown key '" + k + "'");
    return MSSPE_OK;
}

int msspe_kmer_trace(msspe_ctx *ctx, uint32_t *out, int capacity, int *n_out)
{
    if (!ctx || !n_out || capacity < 0 || (capacity && !out)) return MSSPE_ERR_ARG;
    const auto &t = ctx->kmer.trace();
    *n_out = (int)t.size();
    for (int i = 0; i < capacity && i < (int)t.size(); ++i) out[i] = t[(size_t)i];
    return MSSPE_OK;
}

void msspe_destroy(msspe_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->own_stream) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->kmer.release();
        ctx->kmer_rev.release();
        ctx->cover.release();
        ctx->tubes.release();
        ctx->graph.release();
        ctx->thin.release();
        ctx->thin_thal.release();
        ctx->select.release();
        ctx->thin_reach.release();
        for (auto &e : ctx->select_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        for (auto &e : ctx->tolerant.ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        ctx->mm_cov.release();
        ctx->cov_thal.release();
        ctx->background.release();
        {
            auto &w = ctx->site_work;
            for (void *q : {(void *)w.sites, (void *)w.list, (void *)w.dg, (void *)w.t, (void *)w.pool,
                            (void *)w.counts, (void *)w.slab_count, (void *)w.cls, (void *)w.class_counts})
                if (q) (void)hipFree(q);
        }
        {
            auto &w = ctx->amp_work;
            for (void *q : {(void *)w.keys, (void *)w.key_count, (void *)w.sorted, (void *)w.rec, w.tmp,
                            (void *)w.starts, (void *)w.counts})
                if (q) (void)hipFree(q);
            for (hipEvent_t e : w.ev)
                if (e) (void)hipEventDestroy(e);
        }
        {
            auto &w = ctx->reach_work;
            for (void *q : {(void *)w.planes, (void *)w.tiles, (void *)w.starts, (void *)w.acc})
                if (q) (void)hipFree(q);
            for (hipEvent_t e : w.ev)
                if (e) (void)hipEventDestroy(e);
        }
        if (ctx->ev_rev) (void)hipEventDestroy(ctx->ev_rev);
        if (ctx->stream_rev) {
            (void)hipStreamSynchronize(ctx->stream_rev);
            (void)hipStreamDestroy(ctx->stream_rev);
        }
        for (auto &e : ctx->chem_cache)
        {
            if (e.d_pt) (void)hipFree(e.d_pt);
            if (e.d_ft) (void)hipFree(e.d_ft);
            if (e.d_it) (void)hipFree(e.d_it);
            if (e.d_bt) (void)hipFree(e.d_bt);
            if (e.d_btq) (void)hipFree(e.d_btq);
            if (e.d_st) (void)hipFree(e.d_st);
        }
        if (ctx->wsS) (void)hipFree(ctx->wsS);
        if (ctx->wsH) (void)hipFree(ctx->wsH);
        if (ctx->ovf_list) (void)hipFree(ctx->ovf_list);
        if (ctx->ovf_list2) (void)hipFree(ctx->ovf_list2);
        if (ctx->ovf_count) (void)hipFree(ctx->ovf_count);
        if (ctx->d_ovf_total) (void)hipFree(ctx->d_ovf_total);
        if (ctx->d_reasons) (void)hipFree(ctx->d_reasons);
        if (ctx->d_sorted) (void)hipFree(ctx->d_sorted);
        if (ctx->d_perm) (void)hipFree(ctx->d_perm);
        if (ctx->d_sort_scratch) (void)hipFree(ctx->d_sort_scratch);
        if (ctx->d_ab) (void)hipFree(ctx->d_ab);
        if (ctx->d_tb) (void)hipFree(ctx->d_tb);
        for (auto &ev : ctx->prof_events) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        (void)hipStreamDestroy(ctx->own_stream);
    }
    delete ctx;
}

const char *msspe_last_error(const msspe_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int msspe_set_stream(msspe_ctx *ctx, void *hip_stream)
{
    if (!ctx) return MSSPE_ERR_ARG;
    ctx->stream = (hipStream_t)hip_stream;   // NULL is HIP's default (null) stream
    return MSSPE_OK;
}

int msspe_reset_stream(msspe_ctx *ctx)
{
    if (!ctx) return MSSPE_ERR_ARG;
    ctx->stream = ctx->own_stream;
    return MSSPE_OK;
}

// after a synchronisation: did any stage's hand-over list run past its capacity since the last check?
static int check_list_overrun(msspe_ctx *ctx)
{
    if (!ctx->d_ovf_total) return MSSPE_OK;
    uint64_t flag = 0;
    HIP_TRY(ctx, hipMemcpy(&flag, ctx->d_ovf_total + 1, sizeof flag, hipMemcpyDeviceToHost));
    if (!flag) return MSSPE_OK;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ovf_total + 1, 0, sizeof flag, ctx->stream));
    return fail(ctx, MSSPE_ERR_DEVICE, "a hand-over list was overrun: results of the last screen are incomplete");
}

int msspe_synchronize(msspe_ctx *ctx)
{
    if (!ctx) return MSSPE_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_list_overrun(ctx);
}

int msspe_pack_oligos(const char *ascii, int n, int k, uint64_t *packed_out)
{
    if (!ascii || !packed_out || n < 0) return MSSPE_ERR_ARG;
    if (k < 1 || k > 32) return MSSPE_ERR_K;
    for (int i = 0; i < n; ++i) {
        uint64_t w = 0;
        for (int p = 0; p < k; ++p) {
            uint64_t code;
            switch (ascii[(size_t)i * k + p]) {
            case 'A': case 'a': code = 0; break;
            case 'C': case 'c': code = 1; break;
            case 'G': case 'g': code = 2; break;
            case 'T': case 't': code = 3; break;
            default: return MSSPE_ERR_ARG;
            }
            w |= code << (2 * p);
        }
        packed_out[i] = w;
    }
    return MSSPE_OK;
}

void msspe_unpack_oligo(uint64_t packed, int k, char *ascii_out)
{
    for (int p = 0; p < k; ++p) ascii_out[p] = "ACGT"[(packed >> (2 * p)) & 3];
    ascii_out[k] = 0;
}

// The stages of one screen, chosen by cross_dimer_impl (thal ANY) or cross_dimer_end_impl (thal END1).
struct ChainRoute {
    bool end1;          // the END screen: END1 instantiations of every stage and the t decision
    FirstStage first;   // Dense: the dense kernel takes the whole block; Int (ANY only) stands for the integer kernel and
                        // its row-specialised and bound instances until settle_first_stage has picked one
    bool bound_list = false;   // Bound, BoundMirror: the bound list stage runs at every flush (option pair_bound_list)
    bool bound_packed = false; // Bound, BoundMirror: the packed instance is the first stage (option pair_bound_packed)
    bool bound_window = false; // ... and of it the windowed instance (option pair_bound_window; needs bound_list)
    bool bound_list_packed = false; // bound_list behind bound_packed: the list stage's packed instance (option pair_bound_list_packed)
    StageList behind;   // the list stages behind a first stage other than Dense, in order
};

// option pair_bound = auto without a record for this chemistry, threshold and length (ChemEntry::bound_share): one probe
// launch over the head of the call's own block, behind the column sort (it counts its survivors and writes nothing
// else), and one counter read -- the only host round trip the bound adds, once per record.  A stream that is being
// captured cannot be waited for: no record.
static int probe_bound_share(msspe_ctx *ctx, ChemEntry *ce, const ScreenBlock &b)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) (void)hipGetLastError();
    if (cs != hipStreamCaptureStatusNone) return MSSPE_OK;
    const int col1 = (int)std::min<long>(b.sinks.ncols, kBoundProbePairs);
    const int row1 = (int)std::min<long>(b.row1, (long)b.row0 + std::max(1L, kBoundProbePairs / col1));
    PairKernelArgs a = first_stage_args(ctx, ce, b, Launch{b.row0, row1, 0, col1, 0, 0, false});
    a.overflow_list = nullptr;   // no list: the kernel only counts
    unsigned long long *probe = ctx->d_reasons + kBoundSurvivors + 1;
    HIP_TRY(ctx, hipMemsetAsync(probe, 0, sizeof *probe, ctx->stream));
    HIP_TRY(ctx, launch_pairs_bound(a, ce->d_it, ce->d_bt, probe, nullptr, ctx->n_cu, ctx->stream));
    unsigned long long n_surv = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_surv, probe, sizeof n_surv, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ce->bound_share[b.k] = (float)((double)n_surv / ((double)(row1 - b.row0) * (double)col1));
    return MSSPE_OK;
}

// Which instance of the integer first stage takes the block: called once the hand-over lists are sized and the columns
// sorted.  The row-specialised first stage, and in front of the list stages instead of it the BOUND instance where the
// call asks for decisions only (no plane, no edge values): it proves most pairs free of a conflict at about half the
// price and hands the rest to list 0 (thal_pairs_row.hip k_pairs_bound; option pair_bound).
// BoundMirror: a square same-pool block under strand-symmetric tables (ChemEntry::mirror_ok) -- the bound of (a, b)
// stands for (b, a) as well ("Screen each unordered pair once"), so the bound stage fills each unordered
// pair once (screen_plan.hpp cuts its launches).
static int settle_first_stage(msspe_ctx *ctx, ChemEntry *ce, const ScreenBlock &b, ChainRoute &route)
{
    const int k = b.k;
    if (route.first != FirstStage::Int) return MSSPE_OK;
    const bool row_stage = ce->row_ok && k <= pairs_row_max_k() && ctx->opt.pair_kernel != 2 &&
                           (k > pairs_row_oob_max_k() || (ctx->lds_reads_zero && ctx->opt.row_oob));
    if (!row_stage) return MSSPE_OK;
    route.first = FirstStage::Row;
    bool bound_stage = !route.end1 && k <= pairs_bound_max_k() && ce->bound_ok && ctx->opt.pair_bound != 0 &&
                       !b.sinks.dg && !b.sinks.tm && !b.sinks.edge_count;
    if (bound_stage && ctx->opt.pair_bound == 2) {
        if (ce->bound_share[k] < 0.f)
            if (int rc = probe_bound_share(ctx, ce, b)) return rc;
        bound_stage = ce->bound_share[k] >= 0.f && ce->bound_share[k] <= kBoundShareMax;
    }
    if (!bound_stage) return MSSPE_OK;
    const bool mirror = ce->mirror_ok && ctx->opt.pair_mirror != 0 && k == b.k2 && b.row0 == b.col0 && b.row1 == b.col1 &&
                        (long)b.sinks.ncols <= mirror_launch_cap(ctx->list_cap);
    route.first = mirror ? FirstStage::BoundMirror : FirstStage::Bound;
    route.bound_list = ctx->opt.pair_bound_list != 0;
    // the packed instance wherever the chemistry's range fits its field (auto and 1 alike: never where it is not proven);
    // the probe above and the plane form msspe_cross_dimer_bound_dev stay on the exact-unit instance
    route.bound_packed = ce->packed_ok && ctx->opt.pair_bound_packed != 0;
    // of it the windowed instance, whose survivors are list U's to bound: without the bound list stage they would reach the
    // exact chain at its price, so the packed instance stays.  A screen that is being captured keeps the packed instance
    // as well; the probe above and the plane forms never run this one.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) (void)hipGetLastError();
    const long n_pairs = (long)(b.row1 - b.row0) * (long)b.sinks.ncols;
    route.bound_window = route.bound_packed && route.bound_list && ce->window_ok && cs == hipStreamCaptureStatusNone &&
                         (ctx->opt.pair_bound_window == 1 || (ctx->opt.pair_bound_window == 2 && n_pairs >= kWindowAutoMinPairs));
    // The bound list stage's packed instance, behind the packed or the windowed first stage only: list U then meets the very
    // bound (unit and cull rule) the packed first stage applies to the lanes it keeps.  auto: from the window's pair count --
    // below it list U is a few thousand entries, the flush is launch latency, and the finer exact-unit bound costs nothing.
    route.bound_list_packed = route.bound_list && route.bound_packed &&
                              (ctx->opt.pair_bound_list_packed == 1 ||
                               (ctx->opt.pair_bound_list_packed == 2 && n_pairs >= kWindowAutoMinPairs));
    return MSSPE_OK;
}

// Runs a routed screen over the block: the column sort, the first stage over the launches screen_plan.hpp cuts the
// block into, and the hand-over lists flushed through route.behind (ListChain) where the plan says so.
static int run_chain(msspe_ctx *ctx, ChemEntry *ce, ChainRoute route, const ScreenBlock &b)
{
    const bool end1 = route.end1;
    const int ncols = b.sinks.ncols, words = b.sinks.words;
    int rc = 0;
    if ((rc = ensure_workspace(ctx, (size_t)b.k * (size_t)b.k2))) return rc;
    if ((rc = ensure_overflow(ctx, (long)(b.row1 - b.row0) * (long)ncols))) return rc;

    // the conflict bitmap is produced with atomic ORs: clear the caller's block first
    if (b.sinks.bitmap)
        HIP_TRY(ctx, hipMemsetAsync(b.sinks.bitmap, 0, sizeof(uint64_t) * (size_t)(b.row1 - b.row0) * (size_t)words,
                                    ctx->stream));
    GenericDimerArgs g = dimer_args(ctx, ce, b, end1 ? kModeEnd1 : kModeAny);
    if (route.first == FirstStage::Dense) {
        // generic kernel over the whole block, a band of rows per launch (matrix mode derives
        // (row, col) from sinks.row0 / sinks.col0, so the output base pointers move with the band)
        for (const Launch &l : plan_screen(route.first, b.row0, b.row1, b.col0, ncols, ctx->list_cap).launches) {
            GenericDimerArgs gb = g;
            gb.sinks.row0 = l.row0;
            gb.n_work = l.pairs;
            const size_t roff = (size_t)(l.row0 - b.row0);
            if (gb.sinks.bitmap) gb.sinks.bitmap += roff * (size_t)words;
            if (gb.sinks.dg) gb.sinks.dg += roff * (size_t)ncols;
            if (gb.sinks.tm) gb.sinks.tm += roff * (size_t)ncols;
            HIP_TRY(ctx, launch_dimer_generic(gb, ctx->stream, end1));
        }
        return MSSPE_OK;
    }
    if (route.first != FirstStage::Wave) {
        if ((rc = ensure_sort(ctx, (size_t)ncols))) return rc;
        HIP_TRY(ctx, sort_columns_by_composition(b.pool, b.col0, ncols, b.k2, ctx->d_sort_scratch,
                                                 ctx->sort_scratch_bytes, ctx->d_sorted, ctx->d_perm,
                                                 ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, kOvfCounters * sizeof(uint32_t), ctx->stream));
    if ((rc = settle_first_stage(ctx, ce, b, route))) return rc;
    const ScreenPlan plan = plan_screen(route.first, b.row0, b.row1, b.col0, ncols, ctx->list_cap);
    // List 0 (ovf_list) = what the first stage did not answer.
    // The bound list stage (option pair_bound_list; thal_pairs_bound_list.hip): where it is on, the bound first stage
    // appends the lanes that leave it without a bound of their own to list U -- ovf_list2 with its own counter, once per
    // unordered pair -- and a flush first bounds U, appending what it cannot cull to list 0 behind the first stage's
    // entries; the route then runs from list 0 as ever, with ovf_list2, which U has vacated by then (same stream), as its
    // first output list.  Capacity: a launch that processes P pairs appends at most P entries to U and, to list 0, at
    // most P (2 P mirrored) from the two stages together -- an entry of U becomes at most one (two) of list 0 -- which
    // is what the plan's list_entries budget against the capacity already.
    uint2 *const u_list = route.bound_list ? ctx->ovf_list2 : nullptr;
    uint32_t *const u_count = ctx->ovf_count + kOvfU;
    auto flush = [&]() -> int {
        PairKernelArgs a = pair_args(ctx, ce, b);
        if (route.bound_list) {
            a.overflow_list = ctx->ovf_list;
            a.overflow_count = ctx->ovf_count;
            a.overflow_cap = (uint32_t)ctx->list_cap;
            HIP_TRY(ctx, launch_pairs_bound_list(a, ce->d_bt, u_list, u_count, ctx->d_reasons + kBoundListStats, nullptr,
                                                 ctx->n_cu, ctx->stream, route.bound_list_packed ? ce->d_btq : nullptr,
                                                 ce->packed_bias, ce->packed_shift));
        }
        return ListChain(ctx, ce, end1, ctx->ovf_list, ctx->list_cap).run(route.behind, a, g, true);
    };
    auto prof_begin = [&]() -> int {
        if (!ctx->prof_on) return MSSPE_OK;
        if (ctx->prof_used == ctx->prof_events.size()) {
            hipEvent_t e0, e1;
            HIP_TRY(ctx, hipEventCreate(&e0));
            HIP_TRY(ctx, hipEventCreate(&e1));
            ctx->prof_events.emplace_back(e0, e1);
        }
        HIP_TRY(ctx, hipEventRecord(ctx->prof_events[ctx->prof_used].first, ctx->stream));
        return MSSPE_OK;
    };
    auto prof_end = [&]() -> int {
        if (ctx->prof_on) HIP_TRY(ctx, hipEventRecord(ctx->prof_events[ctx->prof_used++].second, ctx->stream));
        return MSSPE_OK;
    };
    for (const Launch &l : plan.launches) {
        if (l.flush_before && (rc = flush())) return rc;
        const PairKernelArgs a = first_stage_args(ctx, ce, b, l);
        if ((rc = prof_begin())) return rc;
        switch (route.first) {
        case FirstStage::Dense: break;   // (returned above)
        case FirstStage::Wave: HIP_TRY(ctx, launch_pairs_wave(a, ce->d_st, nullptr, nullptr, ctx->stream, end1)); break;
        case FirstStage::Split:
            HIP_TRY(ctx, launch_pairs_split(a, ce->d_st, ctx->d_reasons, ctx->opt.split_lanes, ctx->stream));
            break;
        case FirstStage::Fast: HIP_TRY(ctx, launch_pairs_fast(a, ctx->stream, end1)); break;
        case FirstStage::Int: HIP_TRY(ctx, launch_pairs_int(a, ce->d_it, ctx->d_reasons, ctx->n_cu, ctx->stream)); break;
        case FirstStage::Row: HIP_TRY(ctx, launch_pairs_row(a, ce->d_it, ctx->d_reasons, ctx->n_cu, ctx->stream)); break;
        case FirstStage::Bound:
        case FirstStage::BoundMirror:
            HIP_TRY(ctx, launch_pairs_bound(a, ce->d_it, ce->d_bt, ctx->d_reasons + kBoundSurvivors, nullptr, ctx->n_cu,
                                            ctx->stream, route.first == FirstStage::BoundMirror, u_list, u_count,
                                            route.bound_packed ? ce->d_btq : nullptr, ce->packed_bias, ce->packed_shift,
                                            route.bound_window ? &ce->window : nullptr, ctx->d_reasons + kBoundWindowSurvivors));
            break;
        }
        if ((rc = prof_end())) return rc;
    }
    ctx->bound_mirrored += plan.mirrored;
    // every launch leaves pairs pending, and a flush is always followed by a launch: the lists are never empty here
    return plan.launches.empty() ? MSSPE_OK : flush();
}

// What both screens check first, and the chemistry's cache entry of the screen's kind; *ce stays null for an empty
// block (nothing to do).
static int open_screen(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, float threshold, int kind,
                       ChemEntry **ce)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!b.pool || !chem || b.n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (b.k < 2 || b.k > 32 || b.k2 < 2 || b.k2 > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (b.row0 < 0 || b.row1 > b.n || b.row0 > b.row1 || b.col0 < 0 || b.col1 > b.n || b.col0 > b.col1)
        return fail(ctx, MSSPE_ERR_ARG, "row/column range outside the pool");
    if (b.row0 == b.row1 || b.col0 == b.col1) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return chem_entry(ctx, *chem, threshold, ce, kind);
}

// The ANY screen (thal ANY for every ordered pair of the block, conflict iff dG <= the threshold's cut).
static int cross_dimer_impl(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, float dg_threshold)
{
    ChemEntry *ce = nullptr;
    const int rc = open_screen(ctx, b, chem, dg_threshold, kCutAnyDg, &ce);
    if (rc || !ce) return rc;
    const int k = b.k, k2 = b.k2;
    // long oligos: exact-integer kernel with a pair's table split over lanes (honours max_loop)
    // (also short oligos under a loop-size limit the register-table kernels do not implement)
    // Row and column oligos of different lengths (k2 != k) take the rectangular chain: the split-table kernel
    // where the longer of the two is within its proven range (a k x k2 table lies inside the square of its longer
    // side, whose int32 bounds build_split_tables checked), else the wave kernel in matrix mode; then the wave
    // list stage and the dense kernel.  split_min_k and pair_kernel do not apply there: the register-table,
    // integer and row-specialised first stages are square-only.
    const bool rect = k2 != k;
    const int kmax = std::max(k, k2);
    const bool split = !ctx->opt.force_generic && kmax <= ce->split_max_k &&
                       (rect || (!(ctx->opt.pair_kernel == 1) && (k >= ctx->opt.split_min_k || chem->max_loop < 2 * k - 4)));
    // f64, one wave per pair: behind the split kernel, and as the first stage where neither the split
    // kernel nor the register-table chain applies (29 .. 32 bases, parameter files off the grid)
    const bool wave = wave_ok(ctx, ce, kmax);
    const bool wave_matrix = wave && !split && (rect || k > pairs_fast_max_k() || chem->max_loop < 2 * k - 4);
    const bool int_stage = !split && ce->int_ok && !(ctx->opt.pair_kernel == 1);
    ChainRoute route;
    route.end1 = false;
    // the register-table / integer / row first stages are square-only: a rectangle that neither the split nor the
    // wave kernel takes goes to the dense kernel
    if (wave_matrix) route.first = FirstStage::Wave;
    else if (split) route.first = FirstStage::Split;
    else if (rect || !reg_tables_ok(ctx, ce, k)) route.first = FirstStage::Dense;
    else route.first = int_stage ? FirstStage::Int : FirstStage::Fast;   // Int: settle_first_stage picks the instance
    StageList &s = route.behind;
    if (split || wave_matrix) {
        // long oligos: what the split kernel handed on is answered in f64 by one wave per pair; the dense kernel
        // takes what is left (two self-complementary oligos, huge tables)
        if (split && wave) s.add(ListStage::Wave);
    } else if (int_stage) {
        s.add(ListStage::IntList);
        // small screens (the reference's are at most 2,000^2): the short chain.  What the integer list stage leaves
        // (some ten thousand pairs) goes straight to one wave per pair -- each of the three register-table stages
        // in between has a latency floor of 0.4 ... 0.6 ms whatever its list holds, the wave kernel takes 0.13 ms +
        // 16 ns per pair
        if (wave && ctx->opt.short_chain && (long)(b.row1 - b.row0) * (long)(b.col1 - b.col0) <= (1L << 23)) {
            s.add(ListStage::Wave);
        } else {
            if (ce->split_max_k >= k && ctx->opt.split_list) s.add(ListStage::SplitList);
            s.add(ListStage::MainList);
            s.add(ListStage::Wide);
            if (wave) s.add(ListStage::Wave);
        }
    } else {   // pair_kernel "f64", or tables without an integer image: k_pairs_fast first
        s.add(ListStage::Wide);
        if (wave) s.add(ListStage::Wave);
    }
    s.add(ListStage::Dense);
    return run_chain(ctx, ce, route, b);
}

// The END screen (thal END1 for every ordered pair of the block, conflict iff round_fixed_f32(max(0, t), 2) >=
// tm_threshold): the f64 kernels only.  Equal lengths within the register-table kernels' conditions: k_pairs_fast
// END1 over composition-sorted columns, then the wide list, the wave list and the dense kernel; everything else
// (longer oligos, rectangles, small max_loop): the wave kernel in matrix mode where max(k, k2) is within its range,
// then the dense kernel; where neither first stage applies, the dense kernel takes the block.
static int cross_dimer_end_impl(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, float tm_threshold)
{
    ChemEntry *ce = nullptr;
    const int rc = open_screen(ctx, b, chem, tm_threshold, kCutEndT, &ce);
    if (rc || !ce) return rc;
    const bool reg = b.k2 == b.k && reg_tables_ok(ctx, ce, b.k);
    const bool wave = wave_ok(ctx, ce, std::max(b.k, b.k2));
    ChainRoute route;
    route.end1 = true;
    route.first = reg ? FirstStage::Fast : wave ? FirstStage::Wave : FirstStage::Dense;
    if (reg) {
        route.behind.add(ListStage::Wide);
        if (wave) route.behind.add(ListStage::Wave);
    }
    route.behind.add(ListStage::Dense);
    return run_chain(ctx, ce, route, b);
}

// end: the END screen (threshold = tm_threshold) instead of thal ANY
static int cross_dimer_screen(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, float threshold, bool end)
{
    return end ? cross_dimer_end_impl(ctx, b, chem, threshold) : cross_dimer_impl(ctx, b, chem, threshold);
}

int msspe_cross_dimer_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k,
                          const msspe_chem *chem, float dg_threshold, int row0, int row1,
                          int col0, int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap,
                          double *d_dg, double *d_tm)
{
    return cross_dimer_impl(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                              plane_sinks(d_row_conflicts, d_bitmap, d_dg, d_tm)),
                            chem, dg_threshold);
}

// The edge-list forms of the device screens: the count is cleared on the stream the kernels run on.
static int cross_dimer_edges_dev(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, float threshold, bool end)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!b.sinks.edge_count || (b.sinks.edge_cap && !b.sinks.edges))
        return fail(ctx, MSSPE_ERR_ARG, "edge list: null count or buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(b.sinks.edge_count, 0, sizeof(uint64_t), ctx->stream));
    return cross_dimer_screen(ctx, b, chem, threshold, end);
}

int msspe_cross_dimer_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                float dg_threshold, int row0, int row1, int col0, int col1,
                                uint32_t *d_row_conflicts, msspe_edge_dev *d_edges, uint64_t capacity,
                                uint64_t *d_count)
{
    return cross_dimer_edges_dev(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                                   edge_sinks(d_row_conflicts, d_edges, d_count, capacity)),
                                 chem, dg_threshold, false);
}

// Diagnostic: the bound first stage's value for every pair of the block (tests and debugging; no screen reads it).
// with_list: the pairs the first stage would put on list U are bounded by the bound list stage, whose values replace
// their -inf.
static int cross_dimer_bound_plane(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                   float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound, bool with_list,
                                   bool packed = false, bool window = false)   // with_list and packed: both stages' packed instances
{
    const ScreenBlock b = screen_block(d_pool, n, k, k, row0, row1, col0, col1, plane_sinks(nullptr, nullptr, nullptr, nullptr));
    ChemEntry *ce = nullptr;
    const int rc = open_screen(ctx, b, chem, dg_threshold, kCutAnyDg, &ce);
    if (rc || !ce) return rc;
    if (!d_bound) return fail(ctx, MSSPE_ERR_ARG, "msspe_cross_dimer_bound_dev: null output plane");
    if (k > pairs_bound_max_k() || !ce->bound_ok || !ctx->lds_reads_zero || !ctx->opt.row_oob)
        return fail(ctx, MSSPE_ERR_ARG, "msspe_cross_dimer_bound_dev: the bound stage does not apply (more than 13 bases, a cut "
                                        "above 0, tables outside its range, or option row_oob = 0)");
    if (packed && !ce->packed_ok)
        return fail(ctx, MSSPE_ERR_ARG, "msspe_cross_dimer_bound_packed_dev: no coarse unit of the packed instance holds this "
                                        "chemistry's range of cell values");
    if (window && !ce->window_ok)
        return fail(ctx, MSSPE_ERR_ARG, "msspe_cross_dimer_bound_window_dev: the windowed instance does not apply to this chemistry");
    const int ncols = b.sinks.ncols;
    int rc2 = 0;
    const long n_pairs = (long)(row1 - row0) * (long)ncols;
    if ((rc2 = ensure_overflow(ctx, with_list ? n_pairs : 1))) return rc2;   // (the work counter lives beside the list counters)
    if (with_list && n_pairs > ctx->list_cap)
        return fail(ctx, MSSPE_ERR_ARG, "msspe_cross_dimer_bound_list_dev: the block has more pairs than a hand-over list holds");
    if ((rc2 = ensure_sort(ctx, (size_t)ncols))) return rc2;
    HIP_TRY(ctx, sort_columns_by_composition(b.pool, col0, ncols, k, ctx->d_sort_scratch, ctx->sort_scratch_bytes,
                                             ctx->d_sorted, ctx->d_perm, ctx->stream));
    // one launch over the whole block (the diagnostic form appends nothing to list 0)
    const PairKernelArgs a = first_stage_args(ctx, ce, b, Launch{row0, row1, 0, ncols, 0, 0, false});
    if (!with_list) {
        HIP_TRY(ctx, launch_pairs_bound(a, ce->d_it, ce->d_bt, nullptr, d_bound, ctx->n_cu, ctx->stream, false, nullptr, nullptr,
                                        packed ? ce->d_btq : nullptr, ce->packed_bias, ce->packed_shift,
                                        window ? &ce->window : nullptr, nullptr));
        return MSSPE_OK;
    }
    uint32_t *const u_count = ctx->ovf_count + kOvfU;
    HIP_TRY(ctx, hipMemsetAsync(u_count, 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, launch_pairs_bound(a, ce->d_it, ce->d_bt, nullptr, d_bound, ctx->n_cu, ctx->stream, false, ctx->ovf_list2, u_count,
                                    packed ? ce->d_btq : nullptr, ce->packed_bias, ce->packed_shift));
    HIP_TRY(ctx, launch_pairs_bound_list(a, ce->d_bt, ctx->ovf_list2, u_count, nullptr, d_bound, ctx->n_cu, ctx->stream,
                                         packed ? ce->d_btq : nullptr, ce->packed_bias, ce->packed_shift));
    HIP_TRY(ctx, hipMemsetAsync(u_count, 0, sizeof(uint32_t), ctx->stream));
    return MSSPE_OK;
}

int msspe_cross_dimer_bound_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound)
{
    return cross_dimer_bound_plane(ctx, d_pool, n, k, chem, dg_threshold, row0, row1, col0, col1, d_bound, false);
}

int msspe_cross_dimer_bound_packed_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                       float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound)
{
    return cross_dimer_bound_plane(ctx, d_pool, n, k, chem, dg_threshold, row0, row1, col0, col1, d_bound, false, true);
}

int msspe_cross_dimer_bound_window_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                       float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound)
{
    return cross_dimer_bound_plane(ctx, d_pool, n, k, chem, dg_threshold, row0, row1, col0, col1, d_bound, false, true, true);
}

int msspe_cross_dimer_bound_list_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                     float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound)
{
    return cross_dimer_bound_plane(ctx, d_pool, n, k, chem, dg_threshold, row0, row1, col0, col1, d_bound, true);
}

int msspe_cross_dimer_bound_list_packed_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                            float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound)
{
    return cross_dimer_bound_plane(ctx, d_pool, n, k, chem, dg_threshold, row0, row1, col0, col1, d_bound, true, true);
}

double msspe_t_cut(float tm_threshold) { return t_cut(tm_threshold); }

int msspe_cross_dimer_end_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                              float tm_threshold, int row0, int row1, int col0, int col1, uint32_t *d_row_conflicts,
                              uint64_t *d_bitmap, double *d_dg, double *d_tm)
{
    return cross_dimer_end_impl(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                                  plane_sinks(d_row_conflicts, d_bitmap, d_dg, d_tm)),
                                chem, tm_threshold);
}

int msspe_cross_dimer_end_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                    float tm_threshold, int row0, int row1, int col0, int col1,
                                    uint32_t *d_row_conflicts, msspe_end_edge_dev *d_edges, uint64_t capacity,
                                    uint64_t *d_count)
{
    return cross_dimer_edges_dev(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                                   edge_sinks(d_row_conflicts, d_edges, d_count, capacity)),
                                 chem, tm_threshold, true);
}

int msspe_profile_enable(msspe_ctx *ctx, int on)
{
    if (!ctx) return MSSPE_ERR_ARG;
    ctx->prof_on = on != 0;
    ctx->prof_used = 0;
    return MSSPE_OK;
}

int msspe_profile_read(msspe_ctx *ctx, uint64_t *launches, double *total_ms)
{
    if (!ctx || !launches || !total_ms) return MSSPE_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double sum = 0.0;
    for (size_t i = 0; i < ctx->prof_used; ++i) {
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->prof_events[i].first, ctx->prof_events[i].second));
        sum += ms;
    }
    *launches = ctx->prof_used;
    *total_ms = sum;
    ctx->prof_used = 0;
    return MSSPE_OK;
}

int msspe_last_overflow_pairs(msspe_ctx *ctx, uint64_t *count_out)
{
    if (!ctx || !count_out) return MSSPE_ERR_ARG;
    *count_out = 0;
    if (!ctx->d_ovf_total) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t both[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(both, ctx->d_ovf_total, sizeof both, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ovf_total, 0, sizeof both, ctx->stream));
    *count_out = both[0];
    if (both[1]) return fail(ctx, MSSPE_ERR_DEVICE, "a hand-over list was overrun: results of the last screen are incomplete");
    return MSSPE_OK;
}

int msspe_pair_stage_stats(msspe_ctx *ctx, uint64_t out[16])
{
    if (!ctx || !out) return MSSPE_ERR_ARG;
    for (int q = 0; q < 16; ++q) out[q] = 0;
    if (!ctx->d_reasons) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_reasons, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out + 8, ctx->d_reasons + 1033, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_reasons, 0, 9 * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_reasons + 1033, 0, 8 * sizeof(uint64_t), ctx->stream));
    return MSSPE_OK;
}

int msspe_pair_stage_samples(msspe_ctx *ctx, uint64_t *out, int capacity, int *n_out)
{
    if (!ctx || !out || !n_out || capacity < 0) return MSSPE_ERR_ARG;
    *n_out = 0;
    if (!ctx->d_reasons) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t n = 0;
    HIP_TRY(ctx, hipMemcpy(&n, ctx->d_reasons + 8, sizeof n, hipMemcpyDeviceToHost));
    const int m = (int)std::min<uint64_t>(std::min<uint64_t>(n, 1024), (uint64_t)capacity);
    if (m) HIP_TRY(ctx, hipMemcpy(out, ctx->d_reasons + 9, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
    *n_out = m;
    return MSSPE_OK;
}

}  // extern "C"

namespace {

// Host-buffer screens: `packed` (uploaded here) is the pool, the host block's rows [0, row1) against its columns
// [col0, col1).  One pool: columns [0, n).  Pool A + pool B back to back: columns from n_a.  The block's sinks are the
// caller's host buffers, dense over the block as in msspe_cross_dimer.
// end: the END screen (threshold = tm_threshold) instead of thal ANY.
int cross_dimer_host(msspe_ctx *ctx, const std::vector<uint64_t> &packed, const ScreenBlock &host,
                     const msspe_chem *chem, float threshold, bool end)
{
    const size_t n = packed.size(), n_rows = (size_t)host.row1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t words = (size_t)host.sinks.words, nn = n_rows * (size_t)host.sinks.ncols;
    const PairSinks &out = host.sinks;
    DevBuf<uint64_t> d_pool, d_bitmap;
    DevBuf<uint32_t> d_rc;
    DevBuf<double> d_dg, d_tm;
    HIP_TRY(ctx, d_pool.alloc(n));
    HIP_TRY(ctx, hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
    if (out.row_conflicts) {
        HIP_TRY(ctx, d_rc.alloc(n_rows));
        HIP_TRY(ctx, hipMemsetAsync(d_rc, 0, sizeof(uint32_t) * n_rows, ctx->stream));   // on the stream the kernels run on (it is non-blocking: the null stream does not order against it)
    }
    if (out.bitmap) {
        HIP_TRY(ctx, d_bitmap.alloc(n_rows * words));
        HIP_TRY(ctx, hipMemsetAsync(d_bitmap, 0, sizeof(uint64_t) * n_rows * words, ctx->stream));
    }
    if (out.dg) HIP_TRY(ctx, d_dg.alloc(nn));
    if (out.tm) HIP_TRY(ctx, d_tm.alloc(nn));
    int rc = cross_dimer_screen(ctx, screen_block(d_pool, (int)n, host.k, host.k2, 0, host.row1, host.col0, host.col1,
                                                  plane_sinks(d_rc, d_bitmap, d_dg, d_tm)),
                                chem, threshold, end);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_list_overrun(ctx))) return rc;
    if (out.row_conflicts)
        HIP_TRY(ctx, hipMemcpy(out.row_conflicts, d_rc, sizeof(uint32_t) * n_rows, hipMemcpyDeviceToHost));
    if (out.bitmap) HIP_TRY(ctx, hipMemcpy(out.bitmap, d_bitmap, sizeof(uint64_t) * n_rows * words, hipMemcpyDeviceToHost));
    if (out.dg) HIP_TRY(ctx, hipMemcpy(out.dg, d_dg, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (out.tm) HIP_TRY(ctx, hipMemcpy(out.tm, d_tm, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MSSPE_OK;
}

// Host edge lists: the first `have` raw edges (indices already mapped by the caller) sorted by (a, b) as the
// reference's nested loops emit them, with the value Edge::get_dg() yields; MSSPE_ERR_CAPACITY when count > capacity.
// end: END edges (raw t) as msspe_end_edge, t = round_fixed_f32(max(0, t), 2), the SELF_END text value.
int emit_sorted_edges(msspe_ctx *ctx, std::vector<msspe_edge_dev> &raw, uint64_t count, uint64_t capacity,
                      msspe_edge *edges, bool end = false)
{
    std::sort(raw.begin(), raw.end(), [](const msspe_edge_dev &x, const msspe_edge_dev &y) {
        return x.a != y.a ? x.a < y.a : x.b < y.b;
    });
    for (size_t e = 0; e < raw.size(); ++e) {
        edges[e].a = raw[e].a;
        edges[e].b = raw[e].b;
        // what Edge::get_dg() returns: the %g text as f32, stored as "{:.2}", parsed again (delta_g.rs:10-15, 33-46)
        edges[e].dg = end ? round_fixed_f32(raw[e].dg > 0.0 ? raw[e].dg : 0.0, 2)
                          : round_fixed_f32((double)round_g_f32(raw[e].dg), 2);
    }
    if (count > capacity)
        return fail(ctx, MSSPE_ERR_CAPACITY, "edge list: " + std::to_string(count) + " conflict edges, capacity " +
                                                 std::to_string(capacity));
    return MSSPE_OK;
}

// Pool A and pool B back to back in the context's buffer, A first: the single-pool chain then screens rows of A
// against columns n_a + j.
int stage_ab(msspe_ctx *ctx, const uint64_t *d_a, int n_a, const uint64_t *d_b, int n_b)
{
    const size_t need = (size_t)n_a + (size_t)n_b;
    if (ctx->ab_cap < need) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // an earlier screen may still read the old buffer
        if (ctx->d_ab) (void)hipFree(ctx->d_ab);
        ctx->d_ab = nullptr;
        ctx->ab_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_ab, sizeof(uint64_t) * need));
        ctx->ab_cap = need;
    }
    if (n_a)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ab, d_a, sizeof(uint64_t) * (size_t)n_a, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_b)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ab + n_a, d_b, sizeof(uint64_t) * (size_t)n_b, hipMemcpyDeviceToDevice,
                                    ctx->stream));
    return MSSPE_OK;
}

// The screen ran on the staged A + B pool: an edge's b is a pool index, n_a + (B index).
__global__ void k_edges_shift_b(EdgeRecord *edges, const unsigned long long *count, unsigned long long cap,
                                uint32_t shift)
{
    const unsigned long long n = *count < cap ? *count : cap;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (unsigned long long)gridDim.x * blockDim.x)
        edges[e].b -= shift;
}

// ab: the block in the pools' own indices -- rows of A (k = k_a), columns of B (k2 = k_b); its pool and n are those of
// the staged A + B pool and are set here.  end: the END screen (A = oligo 1, the anchored 3' end) instead of thal ANY.
int cross_dimer_ab_impl(msspe_ctx *ctx, const uint64_t *d_a, int n_a, const uint64_t *d_b, int n_b,
                        const ScreenBlock &ab, const msspe_chem *chem, float threshold, bool end)
{
    if (!chem || n_a < 0 || n_b < 0 || (n_a && !d_a) || (n_b && !d_b))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (ab.k < 2 || ab.k > 32 || ab.k2 < 2 || ab.k2 > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (ab.row0 < 0 || ab.row1 > n_a || ab.row0 > ab.row1 || ab.col0 < 0 || ab.col1 > n_b || ab.col0 > ab.col1)
        return fail(ctx, MSSPE_ERR_ARG, "row/column range outside pool A / pool B");
    if ((long)n_a + (long)n_b > (long)INT32_MAX) return fail(ctx, MSSPE_ERR_ARG, "pools too large");
    if (ab.row0 == ab.row1 || ab.col0 == ab.col1) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = stage_ab(ctx, d_a, n_a, d_b, n_b);
    if (rc) return rc;
    // k_a == k_b: the single-pool chain as it is (the 13-mer A x B screen runs on the row kernel); otherwise the
    // rectangular chain
    rc = cross_dimer_screen(ctx, screen_block(ctx->d_ab, n_a + n_b, ab.k, ab.k2, ab.row0, ab.row1, n_a + ab.col0,
                                              n_a + ab.col1, ab.sinks),
                            chem, threshold, end);
    if (rc) return rc;
    if (ab.sinks.edges && ab.sinks.edge_cap && n_a) {
        hipLaunchKernelGGL(k_edges_shift_b, dim3(256), dim3(256), 0, ctx->stream, ab.sinks.edges, ab.sinks.edge_count,
                           ab.sinks.edge_cap, (uint32_t)n_a);
        HIP_TRY(ctx, hipGetLastError());
    }
    return MSSPE_OK;
}

}  // namespace

namespace {

// What a conflict-graph call asks for beyond the block's sinks (row_conflicts, bitmap).  count != null: the edge form.
struct GraphOut {
    uint64_t *kind_counts;
    msspe_kind_edge *edges;
    uint64_t capacity;
    uint64_t *count;
    uint32_t col_first;   // an edge's b for the block's first column (the caller's index space)
};

// What every conflict-graph entry point checks before anything else.
int graph_rule_check(msspe_ctx *ctx, const msspe_chem *chem, const msspe_conflict_rule *rule, const GraphOut &out,
                     bool edge_form)
{
    if (!chem || !rule) return fail(ctx, MSSPE_ERR_ARG, "conflict graph: null chemistry or rule");
    if (!rule->use_any && !rule->use_end) return fail(ctx, MSSPE_ERR_ARG, "conflict graph: the rule enables neither ANY nor END");
    if (edge_form && (!out.count || (out.capacity && !out.edges)))
        return fail(ctx, MSSPE_ERR_ARG, "edge list: null count or buffer");
    return MSSPE_OK;
}

// The block under the rule (msspe_conflict_graph*).  b: the block in pool indices, its sinks the caller's
// row_conflicts and bitmap.  One rule without edges (and with a bitmap to count kinds from, where they are asked for)
// IS that rule's screen on the caller's buffers: the same internal path, so the same route and options.  Otherwise the
// enabled screens fill their planes in the context's scratch a block of rows at a time, and the union, scan and emit
// kernels follow each block; the list's running count (out.count) carries the row bases from block to block.
int conflict_graph_impl(msspe_ctx *ctx, const ScreenBlock &b, const msspe_chem *chem, const msspe_conflict_rule *rule,
                        const GraphOut &out)
{
    // the screens' own argument checks (open_screen), made once and before the edge count is cleared
    if (!b.pool || b.n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (b.k < 2 || b.k > 32 || b.k2 < 2 || b.k2 > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (b.row0 < 0 || b.row1 > b.n || b.row0 > b.row1 || b.col0 < 0 || b.col1 > b.n || b.col0 > b.col1)
        return fail(ctx, MSSPE_ERR_ARG, "row/column range outside the pool");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (out.count) HIP_TRY(ctx, hipMemsetAsync(out.count, 0, sizeof(uint64_t), ctx->stream));
    if (b.row0 == b.row1 || b.col0 == b.col1) return MSSPE_OK;
    const bool any = rule->use_any != 0, end = rule->use_end != 0;
    const int words = b.sinks.words, n_rows = b.row1 - b.row0;
    uint32_t *const row_conflicts = b.sinks.row_conflicts;
    uint64_t *const bitmap = b.sinks.bitmap;
    unsigned long long *const kinds = reinterpret_cast<unsigned long long *>(out.kind_counts);
    if (any != end && !out.count && (bitmap || !kinds)) {
        if (int rc = cross_dimer_screen(ctx, b, chem, end ? rule->end_tm_threshold : rule->dg_threshold, end)) return rc;
        if (kinds)   // every set bit is of the one kind
            HIP_TRY(ctx, launch_graph_union(any ? bitmap : nullptr, end ? bitmap : nullptr, n_rows, words, nullptr, nullptr,
                                            nullptr, kinds, ctx->stream));
        return MSSPE_OK;
    }
    const int block_rows = graph_block_rows(ctx->opt.conflict_graph_block_rows, n_rows, words);
    {
        std::string err;
        if (int rc = ctx->graph.ensure(block_rows, words, ctx->stream, err)) return fail(ctx, rc, err);
    }
    uint64_t *const p_any = any ? ctx->graph.plane(0) : nullptr, *const p_end = end ? ctx->graph.plane(1) : nullptr;
    for (int r0 = b.row0; r0 < b.row1; r0 += block_rows) {
        const int r1 = (int)std::min<long>((long)r0 + block_rows, b.row1), rows = r1 - r0;
        auto plane_block = [&](uint64_t *plane) {
            return screen_block(b.pool, b.n, b.k, b.k2, r0, r1, b.col0, b.col1, plane_sinks(nullptr, plane, nullptr, nullptr));
        };
        if (any)
            if (int rc = cross_dimer_impl(ctx, plane_block(p_any), chem, rule->dg_threshold)) return rc;
        if (end)
            if (int rc = cross_dimer_end_impl(ctx, plane_block(p_end), chem, rule->end_tm_threshold)) return rc;
        HIP_TRY(ctx, launch_graph_union(p_any, p_end, rows, words,
                                        bitmap ? bitmap + (size_t)(r0 - b.row0) * (size_t)words : nullptr,
                                        row_conflicts ? row_conflicts + r0 : nullptr, ctx->graph.row_count(), kinds,
                                        ctx->stream));
        if (out.count) {
            HIP_TRY(ctx, launch_graph_scan(ctx->graph.row_count(), rows, ctx->graph.row_base(),
                                           reinterpret_cast<unsigned long long *>(out.count), ctx->stream));
            HIP_TRY(ctx, launch_graph_emit(p_any, p_end, rows, words, ctx->graph.row_count(), ctx->graph.row_base(),
                                           (uint32_t)r0, out.col_first, out.edges, out.capacity, ctx->stream));
        }
    }
    return MSSPE_OK;
}

// ab: the block in the pools' own indices, as cross_dimer_ab_impl takes it (whose checks and staging these are).
int conflict_graph_ab_impl(msspe_ctx *ctx, const uint64_t *d_a, int n_a, const uint64_t *d_b, int n_b, const ScreenBlock &ab,
                           const msspe_chem *chem, const msspe_conflict_rule *rule, GraphOut out)
{
    if (n_a < 0 || n_b < 0 || (n_a && !d_a) || (n_b && !d_b)) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (ab.k < 2 || ab.k > 32 || ab.k2 < 2 || ab.k2 > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (ab.row0 < 0 || ab.row1 > n_a || ab.row0 > ab.row1 || ab.col0 < 0 || ab.col1 > n_b || ab.col0 > ab.col1)
        return fail(ctx, MSSPE_ERR_ARG, "row/column range outside pool A / pool B");
    if ((long)n_a + (long)n_b > (long)INT32_MAX) return fail(ctx, MSSPE_ERR_ARG, "pools too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ab.row0 == ab.row1 || ab.col0 == ab.col1) {
        if (out.count) HIP_TRY(ctx, hipMemsetAsync(out.count, 0, sizeof(uint64_t), ctx->stream));
        return MSSPE_OK;
    }
    if (int rc = stage_ab(ctx, d_a, n_a, d_b, n_b)) return rc;
    out.col_first = (uint32_t)ab.col0;
    return conflict_graph_impl(ctx, screen_block(ctx->d_ab, n_a + n_b, ab.k, ab.k2, ab.row0, ab.row1, n_a + ab.col0,
                                                 n_a + ab.col1, ab.sinks),
                               chem, rule, out);
}

// The host forms: `packed` (uploaded here) is the pool, rows [0, n_rows) against its columns [col0, col1) -- one pool:
// [0, n); pool A + pool B back to back: from n_a.  Host outputs are assigned.  edge_form: the ordered list, with the
// MSSPE_ERR_CAPACITY contract of msspe_cross_dimer_edges.
int conflict_graph_host(msspe_ctx *ctx, const std::vector<uint64_t> &packed, int n_rows, int k, int k2, int col0, int col1,
                        const msspe_chem *chem, const msspe_conflict_rule *rule, uint32_t *row_conflicts, uint64_t *bitmap,
                        uint64_t *kind_counts, bool edge_form, msspe_kind_edge *edges, uint64_t capacity, uint64_t *count_out)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = packed.size(), words = ((size_t)(col1 - col0) + 63) / 64, rows = (size_t)n_rows;
    DevBuf<uint64_t> d_pool, d_bitmap, d_kinds, d_count;
    DevBuf<uint32_t> d_rc;
    DevBuf<msspe_kind_edge> d_edges;
    HIP_TRY(ctx, d_pool.alloc(n));
    HIP_TRY(ctx, hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
    if (row_conflicts) {
        HIP_TRY(ctx, d_rc.alloc(rows));
        HIP_TRY(ctx, hipMemsetAsync(d_rc, 0, sizeof(uint32_t) * rows, ctx->stream));
    }
    if (bitmap) HIP_TRY(ctx, d_bitmap.alloc(rows * words));
    if (kind_counts) {
        HIP_TRY(ctx, d_kinds.alloc(3));
        HIP_TRY(ctx, hipMemsetAsync(d_kinds, 0, 3 * sizeof(uint64_t), ctx->stream));
    }
    if (edge_form) {
        HIP_TRY(ctx, d_count.alloc(1));
        if (capacity) HIP_TRY(ctx, d_edges.alloc((size_t)capacity));
    }
    const GraphOut out{d_kinds, d_edges, capacity, d_count, 0u};
    int rc = conflict_graph_impl(ctx, screen_block(d_pool, (int)n, k, k2, 0, n_rows, col0, col1,
                                                   plane_sinks(d_rc, d_bitmap, nullptr, nullptr)),
                                 chem, rule, out);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_list_overrun(ctx))) return rc;
    if (row_conflicts) HIP_TRY(ctx, hipMemcpy(row_conflicts, d_rc, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost));
    if (bitmap) HIP_TRY(ctx, hipMemcpy(bitmap, d_bitmap, sizeof(uint64_t) * rows * words, hipMemcpyDeviceToHost));
    if (kind_counts) HIP_TRY(ctx, hipMemcpy(kind_counts, d_kinds, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (!edge_form) return MSSPE_OK;
    HIP_TRY(ctx, hipMemcpy(count_out, d_count, sizeof *count_out, hipMemcpyDeviceToHost));
    const uint64_t have = std::min<uint64_t>(*count_out, capacity);
    if (have) HIP_TRY(ctx, hipMemcpy(edges, d_edges, sizeof(msspe_kind_edge) * (size_t)have, hipMemcpyDeviceToHost));
    if (*count_out > capacity)
        return fail(ctx, MSSPE_ERR_CAPACITY, "edge list: " + std::to_string(*count_out) + " conflict edges, capacity " +
                                                 std::to_string(capacity));
    return MSSPE_OK;
}

// Rule forms of the graph consumers: the whole-pool bitmap under the rule, or under dg_threshold alone (rule == null:
// msspe_cross_dimer_dev, the call the host-pool forms have always made).
int consumer_screen(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                    const msspe_conflict_rule *rule, float dg_threshold, uint64_t *d_bitmap)
{
    if (!rule) return msspe_cross_dimer_dev(ctx, d_pool, n, k, chem, dg_threshold, 0, n, 0, n, nullptr, d_bitmap, nullptr, nullptr);
    return msspe_conflict_graph_dev(ctx, d_pool, n, k, chem, rule, 0, n, 0, n, nullptr, d_bitmap, nullptr);
}

}  // namespace

extern "C" {

int msspe_conflict_graph_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                             const msspe_conflict_rule *rule, int row0, int row1, int col0, int col1,
                             uint32_t *d_row_conflicts, uint64_t *d_bitmap, uint64_t *d_kind_counts)
{
    if (!ctx) return MSSPE_ERR_ARG;
    const GraphOut out{d_kind_counts, nullptr, 0, nullptr, (uint32_t)col0};
    if (int rc = graph_rule_check(ctx, chem, rule, out, false)) return rc;
    return conflict_graph_impl(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                                 plane_sinks(d_row_conflicts, d_bitmap, nullptr, nullptr)),
                               chem, rule, out);
}

int msspe_conflict_graph_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                   const msspe_conflict_rule *rule, int row0, int row1, int col0, int col1,
                                   uint32_t *d_row_conflicts, uint64_t *d_bitmap, uint64_t *d_kind_counts,
                                   msspe_kind_edge *d_edges, uint64_t capacity, uint64_t *d_count)
{
    if (!ctx) return MSSPE_ERR_ARG;
    const GraphOut out{d_kind_counts, d_edges, capacity, d_count, (uint32_t)col0};
    if (int rc = graph_rule_check(ctx, chem, rule, out, true)) return rc;
    return conflict_graph_impl(ctx, screen_block(d_pool, n, k, k, row0, row1, col0, col1,
                                                 plane_sinks(d_row_conflicts, d_bitmap, nullptr, nullptr)),
                               chem, rule, out);
}

int msspe_conflict_graph_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                                int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule, int row0, int row1,
                                int col0, int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap,
                                uint64_t *d_kind_counts)
{
    if (!ctx) return MSSPE_ERR_ARG;
    const GraphOut out{d_kind_counts, nullptr, 0, nullptr, 0u};
    if (int rc = graph_rule_check(ctx, chem, rule, out, false)) return rc;
    return conflict_graph_ab_impl(ctx, d_a, n_a, d_b, n_b,
                                  screen_block(nullptr, 0, k_a, k_b, row0, row1, col0, col1,
                                               plane_sinks(d_row_conflicts, d_bitmap, nullptr, nullptr)),
                                  chem, rule, out);
}

int msspe_conflict_graph_ab_edges_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b,
                                      int n_b, int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule,
                                      int row0, int row1, int col0, int col1, uint32_t *d_row_conflicts,
                                      uint64_t *d_bitmap, uint64_t *d_kind_counts, msspe_kind_edge *d_edges,
                                      uint64_t capacity, uint64_t *d_count)
{
    if (!ctx) return MSSPE_ERR_ARG;
    const GraphOut out{d_kind_counts, d_edges, capacity, d_count, 0u};
    if (int rc = graph_rule_check(ctx, chem, rule, out, true)) return rc;
    return conflict_graph_ab_impl(ctx, d_a, n_a, d_b, n_b,
                                  screen_block(nullptr, 0, k_a, k_b, row0, row1, col0, col1,
                                               plane_sinks(d_row_conflicts, d_bitmap, nullptr, nullptr)),
                                  chem, rule, out);
}

int msspe_conflict_graph(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                         const msspe_conflict_rule *rule, uint32_t *row_conflicts, uint64_t *bitmap,
                         uint64_t *kind_counts)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, rule, GraphOut{}, false)) return rc;
    if (!pool_ascii || n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (n == 0) return MSSPE_OK;
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    return conflict_graph_host(ctx, packed, n, k, k, 0, n, chem, rule, row_conflicts, bitmap, kind_counts, false, nullptr,
                               0, nullptr);
}

int msspe_conflict_graph_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                               const msspe_conflict_rule *rule, msspe_kind_edge *edges, uint64_t capacity,
                               uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, rule, GraphOut{}, false)) return rc;
    if (!pool_ascii || !count_out || n < 0 || (capacity && !edges))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry/count, or a capacity without a buffer");
    *count_out = 0;
    if (n == 0) return MSSPE_OK;
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    return conflict_graph_host(ctx, packed, n, k, k, 0, n, chem, rule, nullptr, nullptr, nullptr, true, edges, capacity,
                               count_out);
}

int msspe_conflict_graph_ab_edges(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                                  int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule,
                                  msspe_kind_edge *edges, uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, rule, GraphOut{}, false)) return rc;
    if (!count_out || n_a < 0 || n_b < 0 || (n_a && !a_ascii) || (n_b && !b_ascii) || (capacity && !edges))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry/count, or a capacity without a buffer");
    *count_out = 0;
    std::vector<uint64_t> packed;
    if (int rc = pack_ab(ctx, a_ascii, n_a, k_a, b_ascii, n_b, k_b, packed)) return rc;
    if (n_a == 0 || n_b == 0) return MSSPE_OK;
    // the staged pool's columns from n_a: bit 0 of the block is B[0], so an edge's b is a B index as it stands
    return conflict_graph_host(ctx, packed, n_a, k_a, k_b, n_a, n_a + n_b, chem, rule, nullptr, nullptr, nullptr, true, edges,
                               capacity, count_out);
}

int msspe_conflict_cover_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap,
                             int drop_self_pairs, uint8_t *d_deleted, int *n_deleted_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (n_deleted_out) *n_deleted_out = 0;
    if (n < 0 || (n && (!d_pool || !d_bitmap || !d_deleted)))
        return fail(ctx, MSSPE_ERR_ARG, "conflict cover: null pool, bitmap or output");
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (n > kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "conflict cover: " + std::to_string(n) + " oligos, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->cover.run(d_pool, n, k, d_bitmap, drop_self_pairs != 0, d_deleted, n_deleted_out, ctx->n_cu,
                                  ctx->stream, err);
    return rc ? fail(ctx, rc, err) : MSSPE_OK;
}

// rule == null: the screen under dg_threshold alone (msspe_conflict_cover); else under the rule (msspe_conflict_cover_rule)
static int conflict_cover_host(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                               const msspe_conflict_rule *rule, float dg_threshold, int drop_self_pairs,
                               uint8_t *deleted_out, int *n_deleted_out)
{
    if (n_deleted_out) *n_deleted_out = 0;
    if (!pool_ascii || !chem || !deleted_out || n < 0)
        return fail(ctx, MSSPE_ERR_ARG, "conflict cover: null pool, chemistry or output");
    if (n == 0) return MSSPE_OK;
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (n > kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "conflict cover: " + std::to_string(n) + " oligos, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    {   // duplicates before the screen, not after it
        std::vector<uint64_t> s(packed);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            return fail(ctx, MSSPE_ERR_ARG, "conflict cover: the pool holds duplicate oligos");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t words = ((size_t)n + 63) / 64;
    DevBuf<uint64_t> d_pool, d_bitmap;
    DevBuf<uint8_t> d_deleted;
    HIP_TRY(ctx, d_pool.alloc((size_t)n));
    HIP_TRY(ctx, d_bitmap.alloc((size_t)n * words));
    HIP_TRY(ctx, d_deleted.alloc((size_t)n));
    HIP_TRY(ctx, hipMemcpyAsync(d_pool, packed.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice,
                                ctx->stream));
    // the screen's decisions only: the bitmap is all the cover reads
    int rc = consumer_screen(ctx, d_pool, n, k, chem, rule, dg_threshold, d_bitmap);
    if (!rc) rc = msspe_conflict_cover_dev(ctx, d_pool, n, k, d_bitmap, drop_self_pairs, d_deleted, n_deleted_out);
    if (!rc) rc = check_list_overrun(ctx);   // the cover has synchronised the stream
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(deleted_out, d_deleted, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MSSPE_OK;
}

int msspe_conflict_cover(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                         float dg_threshold, int drop_self_pairs, uint8_t *deleted_out, int *n_deleted_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    return conflict_cover_host(ctx, pool_ascii, n, k, chem, nullptr, dg_threshold, drop_self_pairs, deleted_out,
                               n_deleted_out);
}

int msspe_conflict_cover_rule(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                              const msspe_conflict_rule *rule, int drop_self_pairs, uint8_t *deleted_out,
                              int *n_deleted_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (n_deleted_out) *n_deleted_out = 0;
    if (int rc = graph_rule_check(ctx, chem, rule, GraphOut{}, false)) return rc;
    return conflict_cover_host(ctx, pool_ascii, n, k, chem, rule, 0.0f, drop_self_pairs, deleted_out, n_deleted_out);
}

int msspe_conflict_tubes_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap,
                             int drop_self_pairs, int max_tubes, uint8_t *d_tube, int *n_tubes_used_out,
                             int *n_unplaced_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (n_tubes_used_out) *n_tubes_used_out = 0;
    if (n_unplaced_out) *n_unplaced_out = 0;
    if (n < 0 || (n && (!d_pool || !d_bitmap || !d_tube)))
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: null pool, bitmap or output");
    if (max_tubes < 1 || max_tubes > kTubeMax)
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: max_tubes must be 1..64");
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (n > kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: " + std::to_string(n) + " oligos, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->tubes.run(ctx->cover, d_pool, n, k, d_bitmap, drop_self_pairs != 0, max_tubes, d_tube,
                                  n_tubes_used_out, n_unplaced_out, ctx->n_cu, ctx->stream, err);
    return rc ? fail(ctx, rc, err) : MSSPE_OK;
}

// rule == null: msspe_conflict_tubes; else msspe_conflict_tubes_rule (as conflict_cover_host)
static int conflict_tubes_host(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                               const msspe_conflict_rule *rule, float dg_threshold, int drop_self_pairs, int max_tubes,
                               uint8_t *tube_out, int *n_tubes_used_out, int *n_unplaced_out)
{
    if (n_tubes_used_out) *n_tubes_used_out = 0;
    if (n_unplaced_out) *n_unplaced_out = 0;
    if (!pool_ascii || !chem || !tube_out || n < 0)
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: null pool, chemistry or output");
    if (max_tubes < 1 || max_tubes > kTubeMax)
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: max_tubes must be 1..64");
    if (n == 0) return MSSPE_OK;
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (n > kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: " + std::to_string(n) + " oligos, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    {   // duplicates before the screen, not after it
        std::vector<uint64_t> s(packed);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            return fail(ctx, MSSPE_ERR_ARG, "conflict tubes: the pool holds duplicate oligos");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t words = ((size_t)n + 63) / 64;
    DevBuf<uint64_t> d_pool, d_bitmap;
    DevBuf<uint8_t> d_tube;
    HIP_TRY(ctx, d_pool.alloc((size_t)n));
    HIP_TRY(ctx, d_bitmap.alloc((size_t)n * words));
    HIP_TRY(ctx, d_tube.alloc((size_t)n));
    HIP_TRY(ctx, hipMemcpyAsync(d_pool, packed.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice,
                                ctx->stream));
    // the screen's decisions only: the bitmap is all the assignment reads
    int rc = consumer_screen(ctx, d_pool, n, k, chem, rule, dg_threshold, d_bitmap);
    if (!rc)
        rc = msspe_conflict_tubes_dev(ctx, d_pool, n, k, d_bitmap, drop_self_pairs, max_tubes, d_tube, n_tubes_used_out,
                                      n_unplaced_out);
    if (!rc) rc = check_list_overrun(ctx);   // the assignment has synchronised the stream
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(tube_out, d_tube, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MSSPE_OK;
}

int msspe_conflict_tubes(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                         float dg_threshold, int drop_self_pairs, int max_tubes, uint8_t *tube_out,
                         int *n_tubes_used_out, int *n_unplaced_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    return conflict_tubes_host(ctx, pool_ascii, n, k, chem, nullptr, dg_threshold, drop_self_pairs, max_tubes, tube_out,
                               n_tubes_used_out, n_unplaced_out);
}

int msspe_conflict_tubes_rule(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                              const msspe_conflict_rule *rule, int drop_self_pairs, int max_tubes, uint8_t *tube_out,
                              int *n_tubes_used_out, int *n_unplaced_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (n_tubes_used_out) *n_tubes_used_out = 0;
    if (n_unplaced_out) *n_unplaced_out = 0;
    if (int rc = graph_rule_check(ctx, chem, rule, GraphOut{}, false)) return rc;
    return conflict_tubes_host(ctx, pool_ascii, n, k, chem, rule, 0.0f, drop_self_pairs, max_tubes, tube_out,
                               n_tubes_used_out, n_unplaced_out);
}

}  // extern "C"

namespace {

// The end of a host edge-list call, behind its screens: synchronises, checks the hand-over lists and brings back the
// count and the first min(count, capacity) raw edges.
int fetch_edges(msspe_ctx *ctx, const uint64_t *d_count, const msspe_edge_dev *d_edges, uint64_t capacity,
                uint64_t *count_out, std::vector<msspe_edge_dev> &raw)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = check_list_overrun(ctx)) return rc;
    HIP_TRY(ctx, hipMemcpy(count_out, d_count, sizeof *count_out, hipMemcpyDeviceToHost));
    raw.resize((size_t)std::min<uint64_t>(*count_out, capacity));
    if (!raw.empty())
        HIP_TRY(ctx, hipMemcpy(raw.data(), d_edges, sizeof(msspe_edge_dev) * raw.size(), hipMemcpyDeviceToHost));
    return MSSPE_OK;
}

// Host edge lists over the same layout as cross_dimer_host (the block's sinks are not used): edge b = column index
// (pool index - col0).  end: the END screen's edges (emit_sorted_edges).
int cross_dimer_edges_host(msspe_ctx *ctx, const std::vector<uint64_t> &packed, const ScreenBlock &host,
                           const msspe_chem *chem, float threshold, msspe_edge *edges, uint64_t capacity,
                           uint64_t *count_out, bool end)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<uint64_t> d_pool, d_count;
    DevBuf<msspe_edge_dev> d_edges;
    const size_t n = packed.size();
    HIP_TRY(ctx, d_pool.alloc(n));
    HIP_TRY(ctx, hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, d_count.alloc(1));
    if (capacity) HIP_TRY(ctx, d_edges.alloc((size_t)capacity));
    HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
    int rc = cross_dimer_screen(ctx, screen_block(d_pool, (int)n, host.k, host.k2, 0, host.row1, host.col0, host.col1,
                                                  edge_sinks(nullptr, d_edges, d_count, capacity)),
                                chem, threshold, end);
    if (rc) return rc;
    std::vector<msspe_edge_dev> raw;
    if ((rc = fetch_edges(ctx, d_count, d_edges, capacity, count_out, raw))) return rc;
    for (auto &e : raw) e.b -= (uint32_t)host.col0;   // pool index -> column index
    // the kernels append in no particular order
    return emit_sorted_edges(ctx, raw, *count_out, capacity, edges, end);
}

// The ASCII forms of the screens: what msspe_cross_dimer and msspe_cross_dimer_end (end) share, and so on.
// out: the caller's host buffers.
int cross_dimer_ascii(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem, float threshold,
                      const PairSinks &out, bool end)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!pool_ascii || !chem || n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (n == 0) return MSSPE_OK;
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    return cross_dimer_host(ctx, packed, screen_block(nullptr, n, k, k, 0, n, 0, n, out), chem, threshold, end);
}

int cross_dimer_edges_ascii(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                            float threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out, bool end)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!pool_ascii || !chem || !count_out || n < 0 || (capacity && !edges))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry/count, or a capacity without a buffer");
    *count_out = 0;
    if (n == 0) return MSSPE_OK;
    std::vector<uint64_t> packed;
    if (int rc = pack_pool(ctx, pool_ascii, n, k, packed)) return rc;
    return cross_dimer_edges_host(ctx, packed, screen_block(nullptr, n, k, k, 0, n, 0, n, PairSinks{}), chem, threshold,
                                  edges, capacity, count_out, end);
}

// ab: rows [0, n_a) of k_a bases against columns [0, n_b) of k_b bases, as cross_dimer_ab_impl takes them
int cross_dimer_ab_ascii(msspe_ctx *ctx, const char *a_ascii, int n_a, const char *b_ascii, int n_b,
                         const ScreenBlock &ab, const msspe_chem *chem, float threshold, bool end)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!chem || n_a < 0 || n_b < 0 || (n_a && !a_ascii) || (n_b && !b_ascii))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    std::vector<uint64_t> packed;
    if (int rc = pack_ab(ctx, a_ascii, n_a, ab.k, b_ascii, n_b, ab.k2, packed)) return rc;
    if (n_a == 0) return MSSPE_OK;
    if (n_b == 0) {   // no columns: no conflicts
        if (ab.sinks.row_conflicts) std::fill(ab.sinks.row_conflicts, ab.sinks.row_conflicts + n_a, 0u);
        return MSSPE_OK;
    }
    return cross_dimer_host(ctx, packed, screen_block(nullptr, n_a + n_b, ab.k, ab.k2, 0, n_a, n_a, n_a + n_b, ab.sinks),
                            chem, threshold, end);
}

}  // namespace

extern "C" {

int msspe_cross_dimer(msspe_ctx *ctx, const char *pool_ascii, int n, int k,
                      const msspe_chem *chem, float dg_threshold, uint32_t *row_conflicts,
                      uint64_t *bitmap, double *dg, double *tm)
{
    return cross_dimer_ascii(ctx, pool_ascii, n, k, chem, dg_threshold, plane_sinks(row_conflicts, bitmap, dg, tm), false);
}

int msspe_cross_dimer_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                            float dg_threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out)
{
    return cross_dimer_edges_ascii(ctx, pool_ascii, n, k, chem, dg_threshold, edges, capacity, count_out, false);
}

int msspe_cross_dimer_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                             int k_b, const msspe_chem *chem, float dg_threshold, int row0, int row1, int col0,
                             int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap, double *d_dg, double *d_tm)
{
    if (!ctx) return MSSPE_ERR_ARG;
    return cross_dimer_ab_impl(ctx, d_a, n_a, d_b, n_b,
                               screen_block(nullptr, 0, k_a, k_b, row0, row1, col0, col1,
                                            plane_sinks(d_row_conflicts, d_bitmap, d_dg, d_tm)),
                               chem, dg_threshold, false);
}

int msspe_cross_dimer_ab_edges_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b,
                                   int n_b, int k_b, const msspe_chem *chem, float dg_threshold, int row0, int row1,
                                   int col0, int col1, uint32_t *d_row_conflicts, msspe_edge_dev *d_edges,
                                   uint64_t capacity, uint64_t *d_count)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_count || (capacity && !d_edges)) return fail(ctx, MSSPE_ERR_ARG, "edge list: null count or buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
    return cross_dimer_ab_impl(ctx, d_a, n_a, d_b, n_b,
                               screen_block(nullptr, 0, k_a, k_b, row0, row1, col0, col1,
                                            edge_sinks(d_row_conflicts, d_edges, d_count, capacity)),
                               chem, dg_threshold, false);
}

int msspe_cross_dimer_ab(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b, int k_b,
                         const msspe_chem *chem, float dg_threshold, uint32_t *row_conflicts, uint64_t *bitmap,
                         double *dg, double *tm)
{
    return cross_dimer_ab_ascii(ctx, a_ascii, n_a, b_ascii, n_b,
                                screen_block(nullptr, 0, k_a, k_b, 0, n_a, 0, n_b, plane_sinks(row_conflicts, bitmap, dg, tm)),
                                chem, dg_threshold, false);
}

int msspe_cross_dimer_ab_edges(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                               int k_b, const msspe_chem *chem, float dg_threshold, msspe_edge *edges, uint64_t capacity,
                               uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!chem || !count_out || n_a < 0 || n_b < 0 || (n_a && !a_ascii) || (n_b && !b_ascii) || (capacity && !edges))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry/count, or a capacity without a buffer");
    *count_out = 0;
    std::vector<uint64_t> packed;
    if (int rc = pack_ab(ctx, a_ascii, n_a, k_a, b_ascii, n_b, k_b, packed)) return rc;
    if (n_a == 0 || n_b == 0) return MSSPE_OK;
    return cross_dimer_edges_host(ctx, packed, screen_block(nullptr, n_a + n_b, k_a, k_b, 0, n_a, n_a, n_a + n_b, PairSinks{}),
                                  chem, dg_threshold, edges, capacity, count_out, false);
}

int msspe_cross_dimer_end(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                          float tm_threshold, uint32_t *row_conflicts, uint64_t *bitmap, double *dg, double *tm)
{
    return cross_dimer_ascii(ctx, pool_ascii, n, k, chem, tm_threshold, plane_sinks(row_conflicts, bitmap, dg, tm), true);
}

int msspe_cross_dimer_end_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                                float tm_threshold, msspe_end_edge *edges, uint64_t capacity, uint64_t *count_out)
{
    static_assert(sizeof(msspe_end_edge) == sizeof(msspe_edge), "edge record layouts differ");
    return cross_dimer_edges_ascii(ctx, pool_ascii, n, k, chem, tm_threshold, reinterpret_cast<msspe_edge *>(edges),
                                   capacity, count_out, true);
}

int msspe_cross_dimer_end_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                                 int k_b, const msspe_chem *chem, float tm_threshold, int row0, int row1, int col0,
                                 int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap, double *d_dg, double *d_tm)
{
    if (!ctx) return MSSPE_ERR_ARG;
    return cross_dimer_ab_impl(ctx, d_a, n_a, d_b, n_b,
                               screen_block(nullptr, 0, k_a, k_b, row0, row1, col0, col1,
                                            plane_sinks(d_row_conflicts, d_bitmap, d_dg, d_tm)),
                               chem, tm_threshold, true);
}

int msspe_cross_dimer_end_ab(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                             int k_b, const msspe_chem *chem, float tm_threshold, uint32_t *row_conflicts,
                             uint64_t *bitmap, double *dg, double *tm)
{
    return cross_dimer_ab_ascii(ctx, a_ascii, n_a, b_ascii, n_b,
                                screen_block(nullptr, 0, k_a, k_b, 0, n_a, 0, n_b, plane_sinks(row_conflicts, bitmap, dg, tm)),
                                chem, tm_threshold, true);
}

int msspe_cross_dimer_edges_mixed(msspe_ctx *ctx, const char *const *oligos, int n, const msspe_chem *chem,
                                  float dg_threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if ((n && !oligos) || !chem || !count_out || n < 0 || (capacity && !edges))
        return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry/count, or a capacity without a buffer");
    *count_out = 0;
    // group the oligos by length: classes in ascending length, each class contiguous in one packed pool;
    // orig[p] = caller's index of pool entry p
    std::vector<int> len((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!oligos[i]) return fail(ctx, MSSPE_ERR_ARG, "null oligo");
        const size_t l = strnlen(oligos[i], 33);
        if (l < 2 || l > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
        len[i] = (int)l;
    }
    if (n == 0) return MSSPE_OK;
    std::vector<uint32_t> orig((size_t)n);
    for (int i = 0; i < n; ++i) orig[i] = (uint32_t)i;
    std::stable_sort(orig.begin(), orig.end(), [&](uint32_t x, uint32_t y) { return len[x] < len[y]; });
    std::vector<uint64_t> packed((size_t)n);
    for (int p = 0; p < n; ++p)
        if (msspe_pack_oligos(oligos[orig[p]], 1, len[orig[p]], &packed[p]))
            return fail(ctx, MSSPE_ERR_ARG, "pool holds characters other than ACGT");
    std::vector<int> cls_off, cls_len;   // class c: pool entries [cls_off[c], cls_off[c + 1])
    for (int p = 0; p < n; ++p)
        if (p == 0 || len[orig[p]] != len[orig[p - 1]]) {
            cls_off.push_back(p);
            cls_len.push_back(len[orig[p]]);
        }
    cls_off.push_back(n);
    const int n_cls = (int)cls_len.size();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<uint64_t> d_pool, d_count;
    DevBuf<msspe_edge_dev> d_edges;
    HIP_TRY(ctx, d_pool.alloc((size_t)n));
    HIP_TRY(ctx, hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, d_count.alloc(1));
    HIP_TRY(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
    if (capacity) HIP_TRY(ctx, d_edges.alloc((size_t)capacity));
    // one block per (row class, column class), all appending to one list: the blocks of one pool need no staging,
    // and an equal-length block (the diagonal) is the single-pool chain itself
    const PairSinks sinks = edge_sinks(nullptr, d_edges, d_count, capacity);
    for (int r = 0; r < n_cls; ++r)
        for (int c = 0; c < n_cls; ++c)
            if (int rc = cross_dimer_impl(ctx, screen_block(d_pool, n, cls_len[r], cls_len[c], cls_off[r], cls_off[r + 1],
                                                            cls_off[c], cls_off[c + 1], sinks),
                                          chem, dg_threshold))
                return rc;
    std::vector<msspe_edge_dev> raw;
    if (int rc = fetch_edges(ctx, d_count, d_edges, capacity, count_out, raw)) return rc;
    for (auto &e : raw) {   // pool entries -> the caller's indices
        e.a = orig[e.a];
        e.b = orig[e.b];
    }
    return emit_sorted_edges(ctx, raw, *count_out, capacity, edges, false);
}

int msspe_thal_detail_pairs(msspe_ctx *ctx, const char *a_ascii, const char *b_ascii, int n, int k,
                            const msspe_chem *chem, int mode, msspe_thal_detail *out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!a_ascii || !b_ascii || !chem || !out || n < 0 || (mode != 1 && mode != 2))
        return fail(ctx, MSSPE_ERR_ARG, "null argument or unsupported mode (1 = ANY, 2 = END1)");
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    if (n == 0) return MSSPE_OK;
    static_assert(sizeof(msspe_thal_detail) == sizeof(ThalDetail), "detail layouts differ");
    std::vector<uint64_t> packed((size_t)2 * n);
    int rc = msspe_pack_oligos(a_ascii, n, k, packed.data());
    if (!rc) rc = msspe_pack_oligos(b_ascii, n, k, packed.data() + n);
    if (rc) return fail(ctx, rc, "oligos hold characters other than ACGT");
    std::vector<uint2> list((size_t)n);
    for (int i = 0; i < n; ++i) list[(size_t)i] = make_uint2((unsigned)i, (unsigned)(n + i));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ChemEntry *ce = nullptr;
    if ((rc = chem_entry(ctx, *chem, -9000.0f, &ce))) return rc;
    if ((rc = ensure_workspace(ctx, (size_t)k * (size_t)k))) return rc;
    DevBuf<uint64_t> d_pool;
    DevBuf<uint2> d_list;
    DevBuf<ThalDetail> d_det;
    hipError_t e;
    if ((e = d_pool.alloc(2 * (size_t)n)) != hipSuccess || (e = d_list.alloc((size_t)n)) != hipSuccess ||
        (e = d_det.alloc((size_t)n)) != hipSuccess ||
        (e = hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_list, list.data(), sizeof(uint2) * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(ctx, e, "thal detail buffers");
    GenericDimerArgs g = dimer_args(ctx, ce, screen_block(d_pool, 2 * n, k, k, 0, 0, 0, 0, PairSinks{}), mode);
    g.list = d_list;
    g.n_work = n;
    g.detail = d_det;
    e = launch_dimer_generic(g, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_det, sizeof(ThalDetail) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "thal detail");
    return MSSPE_OK;
}

int msspe_oligo_stats_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k,
                          const msspe_chem *chem, double *d_tm, double *d_gc, double *d_self_any,
                          double *d_self_end, double *d_hairpin)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_pool || !chem || n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (k < 2 || k > 32) return fail(ctx, MSSPE_ERR_K, "oligo length must be 2..32");
    // oligotm.c divalent_to_monovalent() returns OLIGOTM_ERROR for a negative divalent or dNTP concentration, the
    // dNTP one tested after "dv == 0 -> dntp = 0" (so dv 0 with any dNTP is valid); a negative monovalent one is
    // refused as well.  (thal's own salt term clamps instead: the cross-dimer entry points accept them.)
    if (!(chem->mv >= 0) || !(chem->dv >= 0) || !(chem->dv == 0 || chem->dntp >= 0))
        return fail(ctx, MSSPE_ERR_ARG, "chemistry: stage B needs mv >= 0, dv >= 0 and (dv == 0 or dntp >= 0)");
    if (n == 0) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // Tm, GC % and HAIRPIN_TH need no pair tables: tables that the dimer calls refuse (MSSPE_ERR_TABLES) still serve them
    ChemEntry *ce = nullptr;
    int rc = MSSPE_OK;
    if ((d_self_any || d_self_end) && (rc = chem_entry(ctx, *chem, -9000.0f, &ce))) return rc;   // threshold unused by the self modes
    if ((rc = ensure_workspace(ctx, (size_t)(k + 1) * (size_t)(k + 1)))) return rc;
    if (d_tm || d_gc)
        HIP_TRY(ctx, launch_oligo_tm(d_pool, n, k, chem->dna_conc, chem->mv, chem->dv, chem->dntp,
                                     d_tm, d_gc, ctx->stream));
    // SELF_ANY / SELF_END (thal ANY / END1 of the oligo with itself): ONE fill of the DP serves both -- END1 is the
    // same fillMatrix with the terminal pick restricted to the last row.  What the reference's loop
    // produces (<= 2,000 oligos per call, main.rs:344): one wave per oligo (thal_pairs_wave.hip), whose latency is a
    // single oligo's.  Large pools: one LANE per oligo through the f64 register-table kernels over the list of (i, i)
    // (thal_pairs.hip, 56 then 72 slots), the wave kernel behind them for larger tables.  The dense kernel, one lane
    // per oligo over a global workspace, takes what is left (self-complementary oligos: another RC constant).
    const bool wave = ce && wave_ok(ctx, ce, k);
    const bool lane_ok = wave && n >= ctx->opt.self_lane_from && reg_tables_ok(ctx, ce, k);
    if (wave && (d_self_any || d_self_end)) {
        if ((rc = ensure_overflow(ctx, n))) return rc;
        if (ctx->list_cap < n) return fail(ctx, MSSPE_ERR_NOMEM, "stage B: no memory for the work lists");
        HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, 8 * sizeof(uint32_t), ctx->stream));
        uint32_t *left = ctx->ovf_count + 3;   // entries of ovf_list2 the dense kernel has to take
        if (lane_ok) {
            HIP_TRY(ctx, launch_self_lists(ce->d_ft, ce->c[0], d_pool, n, k, d_self_any, d_self_end, ctx->ovf_list,
                                           ctx->ovf_list2, ctx->ovf_count, (uint32_t)ctx->list_cap, ctx->stream));
            HIP_TRY(ctx, launch_self_wave(ce->d_st, ce->c[0], d_pool, k, 0, n, d_self_any, d_self_end, ctx->ovf_list,
                                          ctx->ovf_count + 2, ctx->ovf_list2, left, (uint32_t)ctx->list_cap,
                                          ctx->ovf_count + 7, ctx->stream));
        } else {
            HIP_TRY(ctx, launch_self_wave(ce->d_st, ce->c[0], d_pool, k, 0, n, d_self_any, d_self_end, nullptr, nullptr,
                                          ctx->ovf_list2, left, (uint32_t)ctx->list_cap, ctx->ovf_count + 7, ctx->stream));
        }
    }
    const ScreenBlock self = screen_block(d_pool, n, k, k, 0, 0, 0, 0, PairSinks{});   // self mode: no pair sinks
    for (int pass = 0; pass < 2; ++pass) {
        double *dst = pass == 0 ? d_self_any : d_self_end;
        if (!dst) continue;
        GenericDimerArgs g = dimer_args(ctx, ce, self, pass == 0 ? kModeAny : kModeEnd1);
        g.n_work = n;
        g.self_mode = 1;
        g.self_t = dst;
        if (wave) {
            g.list = ctx->ovf_list2;
            g.list_count = ctx->ovf_count + 3;
        }
        HIP_TRY(ctx, launch_dimer_generic(g, ctx->stream));
    }
    if (wave && (d_self_any || d_self_end)) HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, 8 * sizeof(uint32_t), ctx->stream));
    if (d_hairpin) {
        HairpinArgs h;
        h.tb = ctx->d_tb;
        h.c = make_hairpin_consts(chem->mv, chem->dv, chem->dntp, chem->temp_c + 273.15,
                                  chem->max_loop);
        h.pool = d_pool;
        h.k = k;
        h.n_work = n;
        h.out_t = d_hairpin;
        h.wsS = ctx->wsS;
        h.wsH = ctx->wsH;
        h.ws_lanes = kGenericLanes;
        // What the reference's loop produces (<= 2,000 oligos per call, main.rs:344): one wave per oligo with the DP
        // planes in LDS (thal_hairpin_wave.hip), whose latency is a single oligo's.  A pool large enough to give
        // every SIMD several full waves: one LANE per oligo over a global workspace laid out [cell][lane]
        // (kernels_generic.hip) -- measured 1,048,576 13-mers: 7.8 ms against 61.7 ms (the serial exterior-loop pass
        // and traceback run in 64 lanes instead of one); 65,536: 0.51 against 4.05; the crossing is near 8,192.
        // (Option "force_generic" takes the one-lane kernel always.)
        if (ctx->opt.force_generic || k > 32 || n >= kHairpinLaneFrom) HIP_TRY(ctx, launch_hairpin_generic(h, ctx->stream));
        else HIP_TRY(ctx, launch_hairpin_wave(h, ctx->n_cu, ctx->stream));
    }
    return MSSPE_OK;
}

int msspe_oligo_stats(msspe_ctx *ctx, const char *pool_ascii, int n, int k,
                      const msspe_chem *chem, double *tm, double *gc, double *self_any,
                      double *self_end, double *hairpin)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!pool_ascii || !chem || n < 0) return fail(ctx, MSSPE_ERR_ARG, "null pool/chemistry");
    if (n == 0) return MSSPE_OK;
    std::vector<uint64_t> packed;
    int rc = pack_pool(ctx, pool_ascii, n, k, packed);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t *d_pool = nullptr;
    double *d_out = nullptr;
    const size_t nb = sizeof(double) * (size_t)n;
    HIP_TRY(ctx, hipMalloc((void **)&d_pool, sizeof(uint64_t) * (size_t)n));
    hipError_t e = hipMalloc((void **)&d_out, nb * 5);
    if (e != hipSuccess) {
        (void)hipFree(d_pool);
        return hip_fail(ctx, e, "hipMalloc");
    }
    (void)hipMemcpy(d_pool, packed.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice);
    double *host[5] = {tm, gc, self_any, self_end, hairpin};
    double *dev[5];
    for (int q = 0; q < 5; ++q) dev[q] = host[q] ? d_out + (size_t)q * n : nullptr;
    rc = msspe_oligo_stats_dev(ctx, d_pool, n, k, chem, dev[0], dev[1], dev[2], dev[3], dev[4]);
    if (!rc) {
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    }
    for (int q = 0; q < 5 && !rc; ++q)
        if (host[q]) {
            e = hipMemcpy(host[q], dev[q], nb, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = hip_fail(ctx, e, "hipMemcpy");
        }
    (void)hipFree(d_pool);
    (void)hipFree(d_out);
    return rc;
}

// Stage A's one internal path: every msspe_kmer_candidates* entry point is a thin caller of kmer_run (one direction
// on the context's stream), kmer_run_host (the same behind an upload of host rows) or kmer_run_both.  sets == NULL:
// both lists empty.
static const msspe_kmer_sets kNoSets = {nullptr, 0, nullptr, 0};

static bool sets_ok(const msspe_kmer_sets *s)
{
    return !s || (s->n_seed >= 0 && s->n_exclude >= 0 && (s->n_seed == 0 || s->seed) && (s->n_exclude == 0 || s->exclude));
}

// seed_from (msspe_kmer_candidates_tolerant*): the caller seeds the run itself; sets then holds exclusions only.
static int kmer_run(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                    int direction, const msspe_kmer_sets *sets, uint64_t *words_out, uint32_t *freq_out, int capacity,
                    int *n_out, const KmerStage::SeedFrom *seed_from = nullptr)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if ((!view.ascii && !view.packed) || !opt || !words_out || !freq_out || !n_out || capacity < 0 || !sets_ok(sets))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (!sets) sets = &kNoSets;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->kmer.run(view, n_seq, seq_len, *opt, direction, words_out, freq_out, capacity, n_out,
                                 ctx->stream, err, sets->seed, sets->n_seed, sets->exclude, sets->n_exclude, seed_from);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

static int kmer_run_host(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                         int direction, const msspe_kmer_sets *sets, uint64_t *words_out, uint32_t *freq_out,
                         int capacity, int *n_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!sets_ok(sets)) return fail(ctx, MSSPE_ERR_ARG, "null seed or exclusion list");
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t *d = nullptr;
    const size_t bytes = (size_t)n_seq * seq_len;
    HIP_TRY(ctx, hipMalloc((void **)&d, bytes ? bytes : 1));
    hipError_t e = hipMemcpy(d, seqs, bytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? kmer_run(ctx, SeqView{d, nullptr, seq_len}, n_seq, seq_len, opt, direction, sets,
                                        words_out, freq_out, capacity, n_out)
                             : hip_fail(ctx, e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

static int kmer_run_both(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                         const msspe_kmer_sets *fwd, const msspe_kmer_sets *rev, uint64_t *words_fwd,
                         uint32_t *freq_fwd, int *n_fwd, uint64_t *words_rev, uint32_t *freq_rev, int *n_rev,
                         int capacity, const KmerStage::SeedFrom *seed_from_fwd = nullptr,
                         const KmerStage::SeedFrom *seed_from_rev = nullptr)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed || !opt || !words_fwd || !freq_fwd || !n_fwd || !words_rev || !freq_rev || !n_rev || capacity < 0 ||
        !sets_ok(fwd) || !sets_ok(rev))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (!fwd) fwd = &kNoSets;
    if (!rev) rev = &kNoSets;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->stream_rev) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream_rev, hipStreamNonBlocking));
    if (!ctx->ev_rev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_rev, hipEventDisableTiming));
    // the second stream starts behind whatever the context's stream holds (the upload of the alignment)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_rev, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_rev, ctx->ev_rev, 0));
    const SeqView view{nullptr, d_packed, seq_len};
    std::string err0, err1;
    int rc0 = MSSPE_OK, rc1 = MSSPE_OK;
    // The two directions are independent (main.rs:673-690 runs them one after the other); each is a chain of small
    // dependent launches with host round trips, so two host threads on two streams overlap them almost entirely.
    std::thread rev_thread([&]() {
        if (hipSetDevice(ctx->device) != hipSuccess) {
            rc1 = MSSPE_ERR_DEVICE;
            err1 = "hipSetDevice failed";
            return;
        }
        rc1 = ctx->kmer_rev.run(view, n_seq, seq_len, *opt, 1, words_rev, freq_rev, capacity, n_rev, ctx->stream_rev, err1,
                                rev->seed, rev->n_seed, rev->exclude, rev->n_exclude, seed_from_rev);
    });
    rc0 = ctx->kmer.run(view, n_seq, seq_len, *opt, 0, words_fwd, freq_fwd, capacity, n_fwd, ctx->stream, err0,
                        fwd->seed, fwd->n_seed, fwd->exclude, fwd->n_exclude, seed_from_fwd);
    rev_thread.join();
    if (rc0) return fail(ctx, rc0, err0);
    if (rc1) return fail(ctx, rc1, "direction 1: " + err1);
    return MSSPE_OK;
}

int msspe_kmer_candidates_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, int direction, uint64_t *words_out,
                              uint32_t *freq_out, int capacity, int *n_out)
{
    return kmer_run(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, direction, nullptr, words_out, freq_out,
                    capacity, n_out);
}

int msspe_kmer_candidates_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, int direction, uint64_t *words_out,
                                     uint32_t *freq_out, int capacity, int *n_out)
{
    return kmer_run(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, direction, nullptr, words_out,
                    freq_out, capacity, n_out);
}

int msspe_kmer_candidates_seeded_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                            const msspe_kmer_opt *opt, int direction, const uint64_t *seed,
                                            int n_seed, uint64_t *words_out, uint32_t *freq_out, int capacity,
                                            int *n_out)
{
    const msspe_kmer_sets sets = {seed, n_seed, nullptr, 0};
    return kmer_run(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, direction, &sets, words_out,
                    freq_out, capacity, n_out);
}

int msspe_kmer_candidates_sets_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                          const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                          uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out)
{
    return kmer_run(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, direction, sets, words_out,
                    freq_out, capacity, n_out);
}

int msspe_kmer_candidates_both_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                          const msspe_kmer_opt *opt, uint64_t *words_fwd, uint32_t *freq_fwd, int *n_fwd,
                                          uint64_t *words_rev, uint32_t *freq_rev, int *n_rev, int capacity)
{
    return kmer_run_both(ctx, d_packed, n_seq, seq_len, opt, nullptr, nullptr, words_fwd, freq_fwd, n_fwd, words_rev,
                         freq_rev, n_rev, capacity);
}

int msspe_kmer_candidates_both_seeded_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                                 const msspe_kmer_opt *opt, const uint64_t *seed_fwd, int n_fwd_seed,
                                                 const uint64_t *seed_rev, int n_rev_seed, uint64_t *words_fwd,
                                                 uint32_t *freq_fwd, int *n_fwd, uint64_t *words_rev,
                                                 uint32_t *freq_rev, int *n_rev, int capacity)
{
    const msspe_kmer_sets fwd = {seed_fwd, n_fwd_seed, nullptr, 0}, rev = {seed_rev, n_rev_seed, nullptr, 0};
    return kmer_run_both(ctx, d_packed, n_seq, seq_len, opt, &fwd, &rev, words_fwd, freq_fwd, n_fwd, words_rev,
                         freq_rev, n_rev, capacity);
}

int msspe_kmer_candidates_both_sets_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                               const msspe_kmer_opt *opt, const msspe_kmer_sets *fwd,
                                               const msspe_kmer_sets *rev, uint64_t *words_fwd, uint32_t *freq_fwd,
                                               int *n_fwd, uint64_t *words_rev, uint32_t *freq_rev, int *n_rev,
                                               int capacity)
{
    return kmer_run_both(ctx, d_packed, n_seq, seq_len, opt, fwd, rev, words_fwd, freq_fwd, n_fwd, words_rev, freq_rev,
                         n_rev, capacity);
}

size_t msspe_packed_row_words(size_t seq_len) { return SeqView::row_words(seq_len); }

int msspe_kmer_candidates(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                          const msspe_kmer_opt *opt, int direction, uint64_t *words_out,
                          uint32_t *freq_out, int capacity, int *n_out)
{
    return kmer_run_host(ctx, seqs, n_seq, seq_len, opt, direction, nullptr, words_out, freq_out, capacity, n_out);
}

int msspe_kmer_candidates_seeded(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, int direction, const uint64_t *seed, int n_seed,
                                 uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out)
{
    const msspe_kmer_sets sets = {seed, n_seed, nullptr, 0};
    return kmer_run_host(ctx, seqs, n_seq, seq_len, opt, direction, &sets, words_out, freq_out, capacity, n_out);
}

int msspe_kmer_candidates_sets(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                               uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out)
{
    return kmer_run_host(ctx, seqs, n_seq, seq_len, opt, direction, sets, words_out, freq_out, capacity, n_out);
}

int msspe_segment_coverage_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                               const uint64_t *rev_words, int n_rev, uint8_t *hit_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs || !opt || !hit_out || n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const SeqView view{d_seqs, nullptr, seq_len};
    const int rc = ctx->kmer.coverage(view, n_seq, seq_len, *opt, fwd_words, n_fwd, rev_words, n_rev,
                                      hit_out, ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_segment_coverage_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                      const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                                      const uint64_t *rev_words, int n_rev, uint8_t *hit_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed || !opt || !hit_out || n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const SeqView view{nullptr, d_packed, seq_len};
    const int rc = ctx->kmer.coverage(view, n_seq, seq_len, *opt, fwd_words, n_fwd, rev_words, n_rev,
                                      hit_out, ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_segment_coverage(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                           const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                           const uint64_t *rev_words, int n_rev, uint8_t *hit_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_segment_coverage_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, fwd_words, n_fwd, rev_words,
                                    n_rev, hit_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

static int segment_coverage_mm_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                    const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                    uint8_t *best_out, uint32_t *primer_segments_out)
{
    if (!opt || !mm || !best_out || n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->mm_cov.run(view, n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p, fwd_words, n_fwd,
                                   rev_words, n_rev, best_out, primer_segments_out, ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_segment_coverage_mm_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  uint8_t *best_out, uint32_t *primer_segments_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return segment_coverage_mm_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, fwd_words,
                                    n_fwd, rev_words, n_rev, best_out, primer_segments_out);
}

int msspe_segment_coverage_mm_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                         const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                         const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                         uint8_t *best_out, uint32_t *primer_segments_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return segment_coverage_mm_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, fwd_words,
                                    n_fwd, rev_words, n_rev, best_out, primer_segments_out);
}

int msspe_segment_coverage_mm(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              uint8_t *best_out, uint32_t *primer_segments_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_segment_coverage_mm_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, fwd_words, n_fwd, rev_words,
                                       n_rev, best_out, primer_segments_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

// The weighted calls' own argument errors (msspe_panel_thin_weighted*, msspe_panel_select_weighted*): NULL weights,
// and a total over the n_seq * P segments above 2^32 - 1 (a gain must fit the high half of the pick key).  The
// options are checked first, as the sibling checks them, so that P is defined.
static int panel_weights_check(msspe_ctx *ctx, const char *who, const PanelWeights &wts, int n_seq, size_t seq_len,
                               const msspe_kmer_opt &opt, int max_mismatches, int exact_3p, const uint64_t *fwd_words,
                               int n_fwd, const uint64_t *rev_words, int n_rev)
{
    if (wts.weight_all_out) *wts.weight_all_out = 0;
    if (wts.weight_kept_out) *wts.weight_kept_out = 0;
    if (!wts.weights) return fail(ctx, MSSPE_ERR_ARG, std::string(who) + ": null weights (the unweighted call takes none)");
    std::string err;
    long P = 0;
    if (int rc = MismatchCoverage::check(n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words,
                                         n_rev, &P, err))
        return fail(ctx, rc, err);
    uint64_t total = 0;
    const uint64_t limit = 0xFFFFFFFFull;
    for (long s = 0; s < P * n_seq; ++s) total += wts.weights[s];   // at most 2^63 / 2^32 segments would wrap: not reachable
    if (total > limit)
        return fail(ctx, MSSPE_ERR_ARG, std::string(who) + ": the weights add up to " + std::to_string(total) +
                                            ", at most " + std::to_string(limit) + " (a gain is a 32-bit number)");
    return MSSPE_OK;
}

// The cost calls' own argument errors (msspe_panel_thin_cost*, msspe_panel_select_cost*): NULL costs and a cost of 0,
// with the first offending index (forward list, then reverse list) in the message.  The caller has checked n_fwd and
// n_rev.
static int panel_costs_check(msspe_ctx *ctx, const char *who, const PanelCosts &cst, int n_fwd, int n_rev)
{
    if (cst.cost_all_out) *cst.cost_all_out = 0;
    if (cst.cost_kept_out) *cst.cost_kept_out = 0;
    if (!cst.costs) return fail(ctx, MSSPE_ERR_ARG, std::string(who) + ": null costs (the call without costs takes none)");
    for (long p = 0; p < (long)n_fwd + (long)n_rev; ++p)
        if (cst.costs[p] == 0)
            return fail(ctx, MSSPE_ERR_ARG, std::string(who) + ": the cost of primer " + std::to_string(p) +
                                                " is 0, a cost is at least 1");
    return MSSPE_OK;
}

static int panel_thin_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                           const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words,
                           int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                           uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                           long long *covered_all_out, long long *covered_kept_out, const PanelWeights *wts = nullptr,
                           const PanelCosts *cst = nullptr)
{
    if (!opt || !mm || !thin || !keep_out || !order_out || !gain_out || !n_picked_out || n_fwd < 0 || n_rev < 0 ||
        (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "panel thin: null argument");
    if (thin->min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel thin: min_gain must be at least 1");
    if (wts)
        if (int rc = panel_weights_check(ctx, "panel thin", *wts, n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p,
                                         fwd_words, n_fwd, rev_words, n_rev))
            return rc;
    if (cst)
        if (int rc = panel_costs_check(ctx, "panel thin", *cst, n_fwd, n_rev)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->thin.run(ctx->mm_cov, view, n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p,
                                 thin->min_gain, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out,
                                 gain_out, n_picked_out, covered_out, covered_all_out, covered_kept_out,
                                 (size_t)ctx->opt.panel_thin_matrix_max_mb << 20, ctx->n_cu, ctx->stream, err, wts,
                                 cst);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_panel_thin_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                         const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                         const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                         uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                         long long *covered_all_out, long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                           rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out, covered_out,
                           covered_all_out, covered_kept_out);
}

int msspe_panel_thin_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                                long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                           rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out, covered_out,
                           covered_all_out, covered_kept_out);
}

int msspe_panel_thin(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                     const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                     const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                     uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                     long long *covered_all_out, long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd, rev_words,
                              n_rev, forced, keep_out, order_out, gain_out, n_picked_out, covered_out, covered_all_out,
                              covered_kept_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_panel_thin_weighted_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  const uint8_t *forced, const uint32_t *weights, uint8_t *keep_out,
                                  uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                                  long long *covered_all_out, long long *covered_kept_out, uint64_t *weight_all_out,
                                  uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    return panel_thin_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                           rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out, covered_out,
                           covered_all_out, covered_kept_out, &wts);
}

int msspe_panel_thin_weighted_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                         const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                         const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                                         const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                         const uint32_t *weights, uint8_t *keep_out, uint32_t *order_out,
                                         uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                                         long long *covered_all_out, long long *covered_kept_out,
                                         uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    return panel_thin_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                           rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out, covered_out,
                           covered_all_out, covered_kept_out, &wts);
}

int msspe_panel_thin_weighted(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                              const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words,
                              int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                              const uint32_t *weights, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                              int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                              long long *covered_kept_out, uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_weighted_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                                       rev_words, n_rev, forced, weights, keep_out, order_out, gain_out, n_picked_out,
                                       covered_out, covered_all_out, covered_kept_out, weight_all_out, weight_kept_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

// msspe_panel_thin_cost*: the thinning by gain per cost.  Without weights every segment counts 1 and
// the two weight sums are the two covered counts.
static int panel_thin_cost_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, const uint32_t *weights, const uint32_t *costs,
                                uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
                                uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                uint64_t *cost_kept_out)
{
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    const PanelCosts cst = {costs, cost_all_out, cost_kept_out};
    long long all = 0, kept = 0;
    const int rc = panel_thin_view(ctx, view, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd, rev_words, n_rev, forced,
                                   keep_out, order_out, gain_out, n_picked_out, covered_out, &all, &kept,
                                   weights ? &wts : nullptr, &cst);
    if (covered_all_out) *covered_all_out = all;
    if (covered_kept_out) *covered_kept_out = kept;
    if (!weights) {
        if (weight_all_out) *weight_all_out = (uint64_t)all;
        if (weight_kept_out) *weight_kept_out = (uint64_t)kept;
    }
    return rc;
}

int msspe_panel_thin_cost_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              const uint8_t *forced, const uint32_t *weights, const uint32_t *costs, uint8_t *keep_out,
                              uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                              long long *covered_all_out, long long *covered_kept_out, uint64_t *weight_all_out,
                              uint64_t *weight_kept_out, uint64_t *cost_all_out, uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_cost_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd,
                                rev_words, n_rev, forced, weights, costs, keep_out, order_out, gain_out, n_picked_out,
                                covered_out, covered_all_out, covered_kept_out, weight_all_out, weight_kept_out,
                                cost_all_out, cost_kept_out);
}

int msspe_panel_thin_cost_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, const uint32_t *weights, const uint32_t *costs,
                                     uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                     uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
                                     uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                     uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_cost_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words,
                                n_fwd, rev_words, n_rev, forced, weights, costs, keep_out, order_out, gain_out,
                                n_picked_out, covered_out, covered_all_out, covered_kept_out, weight_all_out,
                                weight_kept_out, cost_all_out, cost_kept_out);
}

int msspe_panel_thin_cost(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                          const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                          const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint32_t *weights,
                          const uint32_t *costs, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                          int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                          long long *covered_kept_out, uint64_t *weight_all_out, uint64_t *weight_kept_out,
                          uint64_t *cost_all_out, uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_cost_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd, rev_words,
                                   n_rev, forced, weights, costs, keep_out, order_out, gain_out, n_picked_out,
                                   covered_out, covered_all_out, covered_kept_out, weight_all_out, weight_kept_out,
                                   cost_all_out, cost_kept_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

static int panel_thin_depth_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                 const msspe_thin_depth_opt *thin, const uint64_t *fwd_words, int n_fwd,
                                 const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                                 uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                                 uint8_t *depth_kept_out, long long *counts_out)
{
    if (!opt || !mm || !thin || !keep_out || !order_out || !gain_out || !n_picked_out || n_fwd < 0 || n_rev < 0 ||
        (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "panel thin: null argument");
    if (thin->min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel thin: min_gain must be at least 1");
    if (thin->depth < 1 || thin->depth > 255) return fail(ctx, MSSPE_ERR_ARG, "panel thin: depth must be 1..255");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->thin.run_depth(ctx->mm_cov, view, n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p,
                                       thin->min_gain, thin->depth, fwd_words, n_fwd, rev_words, n_rev, forced,
                                       keep_out, order_out, gain_out, n_picked_out, depth_all_out, depth_kept_out,
                                       counts_out, (size_t)ctx->opt.panel_thin_matrix_max_mb << 20, ctx->n_cu,
                                       ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_panel_thin_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                               const msspe_thin_depth_opt *thin, const uint64_t *fwd_words, int n_fwd,
                               const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                               uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                               uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_depth_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words,
                                 n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out,
                                 depth_all_out, depth_kept_out, counts_out);
}

int msspe_panel_thin_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                      const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                      const msspe_thin_depth_opt *thin, const uint64_t *fwd_words, int n_fwd,
                                      const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                                      uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                      uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_depth_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, thin, fwd_words,
                                 n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out, n_picked_out,
                                 depth_all_out, depth_kept_out, counts_out);
}

int msspe_panel_thin_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                           const msspe_mismatch_opt *mm, const msspe_thin_depth_opt *thin, const uint64_t *fwd_words,
                           int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                           uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                           uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_depth_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, fwd_words, n_fwd, rev_words,
                                    n_rev, forced, keep_out, order_out, gain_out, n_picked_out, depth_all_out,
                                    depth_kept_out, counts_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_device_put(msspe_ctx *ctx, const void *host, size_t bytes, void **device_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!device_out || (bytes && !host)) return fail(ctx, MSSPE_ERR_ARG, "null argument");
    *device_out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, bytes ? bytes : 1));
    const hipError_t e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(ctx, e, "hipMemcpy");
    }
    *device_out = d;
    return MSSPE_OK;
}

static int put_rows_impl(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                         size_t row_len, int pad, bool packed, void **device_out);

int msspe_device_put_rows(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                          size_t row_len, int pad, void **device_out)
{
    return put_rows_impl(ctx, rows, row_bytes, n_rows, row_len, pad, false, device_out);
}

int msspe_device_put_rows_packed(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                                 size_t row_len, void **device_out)
{
    return put_rows_impl(ctx, rows, row_bytes, n_rows, row_len, '-', true, device_out);
}

// packed: the ASCII rows only pass through two 16 MB device chunks; each chunk is packed on the device
// (k_pack_rows: 2-bit bases + validity bit, 3/8 of a byte per column) behind its copy, on the copy stream
static int put_rows_impl(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                         size_t row_len, int pad, bool packed, void **device_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!device_out || n_rows < 0 || (n_rows && (!rows || !row_bytes))) return fail(ctx, MSSPE_ERR_ARG, "null argument");
    *device_out = nullptr;
    for (int r = 0; r < n_rows; ++r)
        if (row_bytes[r] > row_len || (row_bytes[r] && !rows[r])) return fail(ctx, MSSPE_ERR_ARG, "row longer than row_len");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t row_out = packed ? SeqView::row_words(row_len) * sizeof(uint64_t) : row_len;
    const size_t total = row_out * (size_t)n_rows;
    char *d = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d, total ? total : 1));
    if (!total) {
        *device_out = d;
        return MSSPE_OK;
    }
    // two pinned staging buffers: the host fills one (rows copied and padded by a few threads) while
    // the DMA engine drains the other -- no rectangular copy of the whole matrix on the host
    const size_t rows_per_chunk = std::max<size_t>(1, (size_t)(16u << 20) / std::max<size_t>(row_len, 1));
    const size_t chunk_bytes = rows_per_chunk * row_len;
    char *stage[2] = {nullptr, nullptr};
    char *dchunk[2] = {nullptr, nullptr};   // packed: device landing zone of the ASCII chunk
    hipEvent_t drained[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipHostMalloc((void **)&stage[b], chunk_bytes, hipHostMallocDefault);
        if (e == hipSuccess && packed) e = hipMalloc((void **)&dchunk[b], chunk_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&drained[b], hipEventDisableTiming);
    }
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t n_threads = std::min<size_t>({(size_t)hw, 8, rows_per_chunk});
    int turn = 0;
    for (size_t r0 = 0; r0 < (size_t)n_rows && e == hipSuccess; r0 += rows_per_chunk, turn ^= 1) {
        const size_t r1 = std::min<size_t>((size_t)n_rows, r0 + rows_per_chunk);
        e = hipEventSynchronize(drained[turn]);   // the copy that last read this buffer (none: returns at once)
        if (e != hipSuccess) break;
        char *buf = stage[turn];
        auto fill = [&](size_t a, size_t b) {
            for (size_t r = a; r < b; ++r) {
                char *dst = buf + (r - r0) * row_len;
                if (row_bytes[r]) std::memcpy(dst, rows[r], row_bytes[r]);
                std::memset(dst + row_bytes[r], pad, row_len - row_bytes[r]);
            }
        };
        if (n_threads < 2) {
            fill(r0, r1);
        } else {
            std::vector<std::thread> pool;
            for (size_t t = 0; t < n_threads; ++t)
                pool.emplace_back(fill, r0 + (r1 - r0) * t / n_threads, r0 + (r1 - r0) * (t + 1) / n_threads);
            for (auto &th : pool) th.join();
        }
        if (packed) {
            e = hipMemcpyAsync(dchunk[turn], buf, (r1 - r0) * row_len, hipMemcpyHostToDevice, copy);
            if (e == hipSuccess)
                e = launch_pack_rows((const uint8_t *)dchunk[turn], (int)(r1 - r0), row_len,
                                     (uint64_t *)(d + r0 * row_out), copy);
        } else {
            e = hipMemcpyAsync(d + r0 * row_len, buf, (r1 - r0) * row_len, hipMemcpyHostToDevice, copy);
        }
        if (e == hipSuccess) e = hipEventRecord(drained[turn], copy);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(copy);
    for (int b = 0; b < 2; ++b) {
        if (drained[b]) (void)hipEventDestroy(drained[b]);
        if (stage[b]) (void)hipHostFree(stage[b]);
        if (dchunk[b]) (void)hipFree(dchunk[b]);
    }
    if (copy) (void)hipStreamDestroy(copy);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(ctx, e, "msspe_device_put_rows");
    }
    *device_out = d;
    return MSSPE_OK;
}

int msspe_device_free(msspe_ctx *ctx, void *device)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!device) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(device));
    return MSSPE_OK;
}

int msspe_device_get(msspe_ctx *ctx, const void *device, size_t bytes, void *host_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (bytes && (!device || !host_out)) return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (!bytes) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(host_out, device, bytes, hipMemcpyDeviceToHost));
    return MSSPE_OK;
}

// The background as one packed row: the stream (records back to back, one '-' between two) passes 16 MB at a time
// through two pinned buffers and two device landing zones; each chunk is packed on the device behind its copy.  A
// chunk starts at a multiple of 64 columns, so its base and validity words are whole words of the packed row.
int msspe_device_put_stream_packed(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                   int n_records, void **device_out, size_t *total_len_out,
                                   uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!device_out || !total_len_out || n_records < 0 || (n_records && (!records || !record_bytes)))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    *device_out = nullptr;
    *total_len_out = 0;
    uint64_t total = 0;
    for (int r = 0; r < n_records; ++r) {
        if (record_bytes[r] && !records[r]) return fail(ctx, MSSPE_ERR_ARG, "null record");
        if (r) total += 1;   // the separator
        if (record_start_out) record_start_out[r] = total;
        total += record_bytes[r];
        if (total >= (1ull << 32))
            return fail(ctx, MSSPE_ERR_ARG, "the background stream must be shorter than 2^32 columns");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t L = (size_t)total, bw = (L + 31) / 32;
    uint64_t *d = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d, std::max<size_t>(8, SeqView::row_words(L) * sizeof(uint64_t))));
    *total_len_out = L;
    if (!L) {
        *device_out = d;
        return MSSPE_OK;
    }
    const size_t chunk = std::min<size_t>((size_t)16u << 20, (L + 63) & ~(size_t)63);
    char *stage[2] = {nullptr, nullptr};
    char *dchunk[2] = {nullptr, nullptr};
    hipEvent_t drained[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipHostMalloc((void **)&stage[b], chunk, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&dchunk[b], chunk);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&drained[b], hipEventDisableTiming);
    }
    int rec = 0;          // the cursor: the next stream column is column `off` of record `rec`,
    size_t off = 0;       // off == record_bytes[rec] being the separator behind it
    int turn = 0;
    for (size_t c0 = 0; c0 < L && e == hipSuccess; c0 += chunk, turn ^= 1) {
        const size_t len = std::min(chunk, L - c0);
        e = hipEventSynchronize(drained[turn]);   // the copy that last read this buffer (none: returns at once)
        if (e != hipSuccess) break;
        char *buf = stage[turn];
        for (size_t at = 0; at < len;) {
            if (off == record_bytes[rec]) {
                buf[at++] = '-';
                ++rec;
                off = 0;
                continue;
            }
            const size_t take = std::min(len - at, record_bytes[rec] - off);
            std::memcpy(buf + at, records[rec] + off, take);
            at += take;
            off += take;
        }
        e = hipMemcpyAsync(dchunk[turn], buf, len, hipMemcpyHostToDevice, copy);
        if (e == hipSuccess)
            e = launch_pack_stream((const uint8_t *)dchunk[turn], len, d + c0 / 32, d + bw + c0 / 64, copy);
        if (e == hipSuccess) e = hipEventRecord(drained[turn], copy);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(copy);
    for (int b = 0; b < 2; ++b) {
        if (drained[b]) (void)hipEventDestroy(drained[b]);
        if (stage[b]) (void)hipHostFree(stage[b]);
        if (dchunk[b]) (void)hipFree(dchunk[b]);
    }
    if (copy) (void)hipStreamDestroy(copy);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(ctx, e, "msspe_device_put_stream_packed");
    }
    *device_out = d;
    return MSSPE_OK;
}

int msspe_background_sites_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                      const msspe_mismatch_opt *mm, const uint64_t *words, int n, uint64_t *sites_out,
                                      msspe_site *d_sites, uint64_t capacity, uint64_t *d_count)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed || !mm || !sites_out || n < 0 || (n && !words) || (d_sites && !d_count))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = ctx->background.run(d_packed, total_len, k, mm->max_mismatches, mm->exact_3p, words, n, sites_out,
                                       d_sites, capacity, d_count, ctx->n_cu, ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_background_sites(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                           int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, uint64_t *sites_out,
                           msspe_site *sites, uint64_t capacity, uint64_t *count_out, uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!mm || !sites_out || n < 0 || (n && !words) || (sites && !count_out))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (count_out) *count_out = 0;
    void *d = nullptr;
    size_t L = 0;
    int rc = msspe_device_put_stream_packed(ctx, records, record_bytes, n_records, &d, &L, record_start_out);
    if (rc) return rc;
    msspe_site *d_sites = nullptr;   // the list and, behind it, its count
    uint64_t *d_count = nullptr;
    hipError_t e = hipSuccess;
    if (sites) {
        const size_t list_bytes = (sizeof(msspe_site) * (size_t)capacity + 7) & ~(size_t)7;
        e = hipMalloc((void **)&d_sites, list_bytes + sizeof(uint64_t));
        if (e == hipSuccess) {
            d_count = (uint64_t *)((char *)d_sites + list_bytes);
            e = hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream);
        }
    }
    if (e == hipSuccess) {
        rc = msspe_background_sites_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, sites_out, d_sites,
                                               capacity, d_count);
        if (!rc && sites) {
            uint64_t count = 0;
            e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            const uint64_t kept = std::min(count, capacity);
            if (e == hipSuccess && kept) e = hipMemcpy(sites, d_sites, sizeof(msspe_site) * kept, hipMemcpyDeviceToHost);
            if (e == hipSuccess) {
                std::sort(sites, sites + kept, [](const msspe_site &a, const msspe_site &b) {
                    if (a.primer != b.primer) return a.primer < b.primer;
                    if (a.strand != b.strand) return a.strand < b.strand;
                    return a.pos < b.pos;
                });
                *count_out = count;
                if (count > capacity) rc = fail(ctx, MSSPE_ERR_CAPACITY, "site list capacity too small");
            }
        }
    }
    if (d_sites) (void)hipFree(d_sites);
    (void)msspe_device_free(ctx, d);
    if (e != hipSuccess) return hip_fail(ctx, e, "msspe_background_sites");
    return rc;
}

namespace {

// The work list of the thal-scored site passes holds 2^site_list_cap_log2 sites; a pair's column is n + site index in
// 31 bits, which bounds the primers such a pass takes.
size_t site_list_cap(const msspe_ctx *ctx) { return (size_t)1 << ctx->opt.site_list_cap_log2; }
bool site_pool_fits(const msspe_ctx *ctx, int n) { return (uint64_t)n + site_list_cap(ctx) < (1ull << 31); }

int ensure_site_work(msspe_ctx *ctx, size_t cap, int n, int flank)
{
    auto &w = ctx->site_work;
    if (flank && w.cls_cap < cap) {
        if (w.cls) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipFree(w.cls);
        }
        w.cls = nullptr;
        w.cls_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.cls, cap));
        w.cls_cap = cap;
    }
    if (flank && !w.class_counts)
        HIP_TRY(ctx, hipMalloc((void **)&w.class_counts, sizeof(uint32_t) * 2 * kSiteClasses));
    if (w.cap != cap) {
        if (w.sites || w.list || w.dg || w.t) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (void *q : {(void *)w.sites, (void *)w.list, (void *)w.dg, (void *)w.t})
            if (q) (void)hipFree(q);
        w.sites = nullptr;
        w.list = nullptr;
        w.dg = w.t = nullptr;
        w.cap = 0;
        hipError_t e = hipMalloc((void **)&w.sites, sizeof(msspe_site) * cap);
        if (e == hipSuccess) e = hipMalloc((void **)&w.list, sizeof(uint2) * cap);
        if (e == hipSuccess) e = hipMalloc((void **)&w.dg, sizeof(double) * cap);
        if (e == hipSuccess) e = hipMalloc((void **)&w.t, sizeof(double) * cap);
        if (e != hipSuccess) {
            for (void *q : {(void *)w.sites, (void *)w.list, (void *)w.dg, (void *)w.t})
                if (q) (void)hipFree(q);
            w.sites = nullptr;
            w.list = nullptr;
            w.dg = w.t = nullptr;
            return hip_fail(ctx, e, "hipMalloc(site work list)");
        }
        w.cap = cap;
    }
    if (w.pool_cap < (size_t)n + cap) {
        if (w.pool) (void)hipFree(w.pool);
        w.pool = nullptr;
        w.pool_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.pool, sizeof(uint64_t) * ((size_t)n + cap)));
        w.pool_cap = (size_t)n + cap;
    }
    if (w.counts_cap < 4 * (size_t)n) {
        if (w.counts) (void)hipFree(w.counts);
        w.counts = nullptr;
        w.counts_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.counts, sizeof(uint64_t) * 4 * (size_t)n));
        w.counts_cap = 4 * (size_t)n;
    }
    if (!w.slab_count) HIP_TRY(ctx, hipMalloc((void **)&w.slab_count, sizeof(uint64_t)));
    return MSSPE_OK;
}

// thal of the pairs list[0 .. count) -- (primer, n + site index) into the site pool -- by list index into the work
// list's dg / t planes: the register-table list stages where they may take the length and chemistry, the wave list
// stage, the dense kernel, over the caller's list as list 0 (ListChain).  *ovf_count[0] == count (k_site_oligos, or
// the class counter of a flanked call).  k2: the template oligos' length -- k without a flank; a longer template
// (k + fl + fr) is a rectangle, which the register-table stages do not take: one wave per pair where the template is
// within that kernel's range, then the dense kernel.
// The hand-over statistics are the cross-dimer calls': this chain does not feed them.
int score_site_pairs(msspe_ctx *ctx, ChemEntry *ce, bool end1, int n, int k, int k2, uint2 *list, uint32_t count)
{
    auto &w = ctx->site_work;
    // a block without rows or columns whose columns start at n: (row - row0) * ncols + (col - col0) = the site index
    const ScreenBlock b = screen_block(w.pool, n, k, k2, 0, 0, n, n, plane_sinks(nullptr, nullptr, w.dg, w.t));
    GenericDimerArgs g = dimer_args(ctx, ce, b, end1 ? kModeEnd1 : kModeAny);
    PairKernelArgs a = pair_args(ctx, ce, b);
    StageList route;
    if (k2 == k && reg_tables_ok(ctx, ce, k)) {
        route.add(ListStage::MainList);
        route.add(ListStage::Wide);
    }
    if (wave_ok(ctx, ce, std::max(k, k2))) route.add(ListStage::Wave);
    route.add(ListStage::Dense);
    HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count + 1, 0, 7 * sizeof(uint32_t), ctx->stream));
    return ListChain(ctx, ce, end1, list, (long)count).run(route, a, g, false);
}

// Before the first slab of a thal-scored site pass: the chemistry's entry at the threshold (END1 or ANY), the DP
// workspace for k-base primers on templates of k + 2 * flank bases, hand-over lists of the work list's size and the
// work list for n primers (n < 0: none -- a tolerant call makes it per direction, under the mutex).
int site_scoring_begin(msspe_ctx *ctx, const msspe_chem &chem, float tm_threshold, bool end1, int k, int flank, int n,
                       ChemEntry **ce_out)
{
    int rc;
    if ((rc = chem_entry(ctx, chem, tm_threshold, ce_out, end1 ? kCutEndT : kCutAnyT)) ||
        (rc = ensure_workspace(ctx, (size_t)k * (size_t)(k + 2 * flank))) ||
        (rc = ensure_overflow(ctx, (long)site_list_cap(ctx))))
        return rc;
    return n < 0 ? MSSPE_OK : ensure_site_work(ctx, site_list_cap(ctx), n, flank);
}

// The pool "forward words then reverse words" at the head of the work list's pool, where the pairs' rows point, and
// the hand-over counters zeroed.
int upload_site_pool(msspe_ctx *ctx, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev)
{
    auto &w = ctx->site_work;
    if (n_fwd)
        HIP_TRY(ctx, hipMemcpyAsync(w.pool, fwd_words, sizeof(uint64_t) * (size_t)n_fwd, hipMemcpyHostToDevice,
                                    ctx->stream));
    if (n_rev)
        HIP_TRY(ctx, hipMemcpyAsync(w.pool + n_fwd, rev_words, sizeof(uint64_t) * (size_t)n_rev,
                                    hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->ovf_count, 0, 8 * sizeof(uint32_t), ctx->stream));
    return MSSPE_OK;
}

extern "C++" {   // (a std::string and templates, within this file's extern "C" block)

std::string site_list_overrun(const char *pass, uint64_t count, size_t cap)
{
    return std::string(pass) + ": one segment group against one primer has " + std::to_string(count) +
           " matches, the work list holds " + std::to_string(cap) + " (msspe_set_option \"site_list_cap_log2\")";
}

// Behind a synchronisation of a pass that times its phases (st: CoverageThal or PanelThinThal; the last three events
// stand before a slab's scores, after them and after its fold): the listing just made, if one was, and the scores and
// the fold of the slab before it, if `scored` says that they wait to be read.
template <class Stats>
void read_slab_times(Stats &st, bool listed, bool &scored)
{
    const int b = (int)(sizeof st.ev / sizeof st.ev[0]) - 3;
    float l = 0.f, a = 0.f, f = 0.f;
    if (scored && hipEventElapsedTime(&a, st.ev[b], st.ev[b + 1]) == hipSuccess &&
        hipEventElapsedTime(&f, st.ev[b + 1], st.ev[b + 2]) == hipSuccess) {
        st.score_us += (long long)(a * 1000.f);
        st.fold_us += (long long)(f * 1000.f);
    }
    scored = false;
    if (listed && hipEventElapsedTime(&l, st.ev[0], st.ev[1]) == hipSuccess) st.list_us += (long long)(l * 1000.f);
}

// The slab loop of every thal-scored site pass.  A slab, taken from the back of `todo`, is listed into the work list
// and its count read back; one that overran the list is split (slab_split.hpp) and its parts, pushed ascending, are
// listed again; only a slab that fitted is counted, scored in steps of the hand-over lists' size, and folded.
//   list(s): lists slab s, counting into site_work.slab_count, and whatever else the pass reads back with the count
//   synced(): behind the synchronisation that brought the count (the one the loop makes per listed slab)
//   prepare(s, count, n_pairs): before the steps of a slab of `count` matches; n_pairs, preset to count: pairs to score
//   score(c0, cnt): cuts and scores pairs [c0, c0 + cnt);  fold(s, count): folds the slab's scores
//   cannot_split(count): the pass's failure when one outer element against one primer overran the list
template <class List, class Synced, class Prepare, class Score, class Fold, class CannotSplit>
int run_slabs(msspe_ctx *ctx, std::vector<Slab> todo, long long &slabs, long long &redone, long long *matches,
              List list, Synced synced, Prepare prepare, Score score, Fold fold, CannotSplit cannot_split)
{
    auto &w = ctx->site_work;
    const uint64_t cap = site_list_cap(ctx);
    int rc;
    while (!todo.empty()) {
        const Slab s = todo.back();
        todo.pop_back();
        HIP_TRY(ctx, hipMemsetAsync(w.slab_count, 0, sizeof(uint64_t), ctx->stream));
        if ((rc = list(s))) return rc;
        uint64_t count = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&count, w.slab_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        synced();
        if (count > cap) {
            ++redone;
            if (!split_slab(s, count, cap, todo)) return cannot_split(count);
            continue;
        }
        if (!count) continue;
        ++slabs;
        if (matches) *matches += (long long)count;
        uint32_t n_pairs = (uint32_t)count;
        if ((rc = prepare(s, count, n_pairs))) return rc;
        // the hand-over lists may be shorter than the work list (a fixed list_cap_log2, a card short of memory)
        const uint32_t step = (uint32_t)std::min<uint64_t>(n_pairs, (uint64_t)ctx->list_cap);
        for (uint32_t c0 = 0; c0 < n_pairs; c0 += step)
            if ((rc = score(c0, std::min(step, n_pairs - c0)))) return rc;
        if ((rc = fold(s, count))) return rc;
    }
    return MSSPE_OK;
}

}  // extern "C++"

// Room for `need` stable keys: the buffer doubles from 2^amplicon_keys_cap_log2 until it holds them, and the `have`
// keys written so far move over, device to device.
int ensure_amplicon_keys(msspe_ctx *ctx, uint64_t have, uint64_t need)
{
    auto &w = ctx->amp_work;
    if (!w.key_count) HIP_TRY(ctx, hipMalloc((void **)&w.key_count, sizeof(uint64_t)));
    if (w.keys && need <= w.keys_cap) return MSSPE_OK;
    size_t cap = w.keys ? w.keys_cap : (size_t)1 << ctx->opt.amplicon_keys_cap_log2;
    while (cap < need) {
        cap *= 2;
        ++w.grows;
    }
    if (w.keys && cap == w.keys_cap) return MSSPE_OK;
    uint64_t *grown = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&grown, sizeof(uint64_t) * cap));
    hipError_t e = hipSuccess;
    if (w.keys && have)
        e = hipMemcpyAsync(grown, w.keys, sizeof(uint64_t) * have, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && w.keys) e = hipStreamSynchronize(ctx->stream);   // the old buffer's last reader and writer
    if (e != hipSuccess) {
        (void)hipFree(grown);
        return hip_fail(ctx, e, "growing the stable-key buffer");
    }
    if (w.keys) (void)hipFree(w.keys);
    w.keys = grown;
    w.keys_cap = cap;
    return MSSPE_OK;
}

// msspe_background_thal[_flank]_packed_dev, and with keys the same pass for
// msspe_background_amplicons[_flank]_packed_dev: the fold of every slab also appends the keys of its stable sites to
// ctx->amp_work.keys; amp_work.n_keys counts them.  With planes (msspe_stream_reach*, never together with keys) the
// fold ORs every stable site's position into the bit plane of its strand; the caller has cleared the planes.  flank 0: every template oligo is its window, one list per chunk
// (k_site_oligos).  flank > 0: the sites of a chunk are classed by the flanks they found (k_site_oligos_flank), the
// class counters come to the host, their exclusive scan places the classes' runs in the list (k_site_group), and
// each non-empty class is scored as a list of its own with k2 = k + fl + fr.
int background_thal_pass(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                         const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem, int mode,
                         float tm_threshold, int flank, uint64_t *sites_out, uint64_t *stable_out,
                         msspe_scored_site *d_sites, uint64_t capacity, uint64_t *d_count, bool keys,
                         uint64_t *plane_plus = nullptr, uint64_t *plane_minus = nullptr)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed || !mm || !sites_out || !stable_out || !chem || n < 0 || (n && !words) || (d_sites && !d_count))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (mode != 1 && mode != 2) return fail(ctx, MSSPE_ERR_ARG, "background_thal: mode must be 1 (ANY) or 2 (END1)");
    if (k < 2 || k > 31) return fail(ctx, MSSPE_ERR_K, "background_thal: unsupported k (need 2 <= k <= 31)");
    if (flank < 0 || flank > kMaxSiteFlank) return fail(ctx, MSSPE_ERR_ARG, "background_thal: flank must be 0..4");
    if (k + 2 * flank > 32)
        return fail(ctx, MSSPE_ERR_ARG, "background_thal: k + 2 * flank exceeds 32 bases, the longest template oligo");
    std::string err;
    int rc = BackgroundSites::check(total_len, k, mm->max_mismatches, mm->exact_3p, words, n, err);
    if (rc) return fail(ctx, rc, err);
    if (!site_pool_fits(ctx, n)) return fail(ctx, MSSPE_ERR_ARG, "background_thal: too many primers");
    std::fill(sites_out, sites_out + 2 * (size_t)n, (uint64_t)0);
    std::fill(stable_out, stable_out + 2 * (size_t)n, (uint64_t)0);
    auto &w = ctx->site_work;
    auto &aw = ctx->amp_work;
    w.slabs = w.redone = 0;
    w.flank_classes = w.truncated = 0;
    uint32_t classes_seen = 0;   // bit c: a site of class c was scored
    if (keys) aw.n_keys = aw.grows = 0;
    if (n == 0 || total_len < (size_t)k) return MSSPE_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (keys) {   // a buffer an earlier call grew is kept: no result depends on its size
        if ((rc = ensure_amplicon_keys(ctx, 0, 0))) return rc;
        aw.grows = 0;
        HIP_TRY(ctx, hipMemsetAsync(aw.key_count, 0, sizeof(uint64_t), ctx->stream));
    }
    uint64_t n_keys = 0;   // stable keys of the slabs folded so far
    const bool end1 = mode == 2;
    ChemEntry *ce = nullptr;
    if ((rc = site_scoring_begin(ctx, *chem, tm_threshold, end1, k, flank, n, &ce))) return rc;
    const double cut = ce->c[0].g_cut;
    const size_t cap = site_list_cap(ctx);
    if ((rc = ctx->background.prepare(k, words, n, ctx->stream, err))) return fail(ctx, rc, err);
    if ((rc = upload_site_pool(ctx, words, n, nullptr, 0))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(w.counts, 0, sizeof(uint64_t) * 4 * (size_t)n, ctx->stream));

    // Slabs (runs [r0, r1) x primers [p0, p1)), the whole stream first: a slab whose sites do not fit the work list
    // is split -- into as many parts as its count says, by runs while it has several, then by primers -- and its
    // parts are listed again; only a slab that fitted is scored and counted (run_slabs).
    auto list = [&](const Slab &s) -> int {
        if ((rc = ctx->background.list_slab(d_packed, total_len, k, mm->max_mismatches, mm->exact_3p, s.p0, s.p1,
                                            (uint32_t)s.o0, (uint32_t)s.o1, w.sites, cap, w.slab_count, ctx->n_cu,
                                            ctx->stream, err)))
            return fail(ctx, rc, err);
        if (keys)   // behind the last fold in stream order: exact
            HIP_TRY(ctx, hipMemcpyAsync(&n_keys, aw.key_count, sizeof n_keys, hipMemcpyDeviceToHost, ctx->stream));
        return MSSPE_OK;
    };
    auto score = [&](uint32_t c0, uint32_t cnt) -> int {
        if (!flank) {
            HIP_TRY(ctx, launch_site_oligos(d_packed, total_len, k, w.sites, c0, cnt, n, w.pool, w.list + c0,
                                            ctx->ovf_count, ctx->stream));
            classes_seen |= 1u;
            return score_site_pairs(ctx, ce, end1, n, k, k, w.list + c0, cnt);
        }
        uint32_t per_class[kSiteClasses];
        HIP_TRY(ctx, hipMemsetAsync(w.class_counts, 0, sizeof(uint32_t) * 2 * kSiteClasses, ctx->stream));
        HIP_TRY(ctx, launch_site_oligos_flank(d_packed, total_len, k, flank, w.sites, c0, cnt, n, w.pool, w.cls,
                                              w.class_counts, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(per_class, w.class_counts, sizeof per_class, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int n_classes = (flank + 1) * (flank + 1);
        SiteClassOffsets off;
        std::memset(&off, 0, sizeof off);
        uint32_t at = 0;
        for (int c = 0; c < n_classes; ++c) {
            off.at[c] = at;
            at += per_class[c];
        }
        if (at != cnt) return fail(ctx, MSSPE_ERR_DEVICE, "background_thal: the flank classes do not add up");
        HIP_TRY(ctx, launch_site_group(w.sites, c0, cnt, n, w.cls, off, w.class_counts + kSiteClasses, w.list + c0,
                                       ctx->stream));
        for (int c = 0; c < n_classes; ++c) {
            if (!per_class[c]) continue;
            const int fl = c / (flank + 1), fr = c % (flank + 1);
            classes_seen |= 1u << c;
            if (fl < flank || fr < flank) w.truncated += per_class[c];
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ovf_count, w.class_counts + c, sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                        ctx->stream));
            if ((rc = score_site_pairs(ctx, ce, end1, n, k, k + fl + fr, w.list + c0 + off.at[c], per_class[c])))
                return rc;
        }
        return MSSPE_OK;
    };
    auto fold = [&](const Slab &, uint64_t count) -> int {
        if (plane_plus) {
            HIP_TRY(ctx, launch_site_fold_planes(w.sites, (uint32_t)count, w.dg, w.t, cut, n, w.counts, d_sites,
                                                 capacity, d_sites ? d_count : nullptr, plane_plus, plane_minus,
                                                 ctx->stream));
            return MSSPE_OK;
        }
        if (!keys) {
            HIP_TRY(ctx, launch_site_fold(w.sites, (uint32_t)count, w.dg, w.t, cut, n, w.counts, d_sites, capacity,
                                          d_sites ? d_count : nullptr, ctx->stream));
            return MSSPE_OK;
        }
        if ((rc = ensure_amplicon_keys(ctx, n_keys, n_keys + count))) return rc;
        HIP_TRY(ctx, launch_site_fold_keys(w.sites, (uint32_t)count, w.dg, w.t, cut, n, w.counts, d_sites, capacity,
                                           d_sites ? d_count : nullptr, aw.keys, aw.keys_cap, aw.key_count,
                                           ctx->stream));
        return MSSPE_OK;
    };
    auto cannot_split = [&](uint64_t) {
        return fail(ctx, MSSPE_ERR_DEVICE, "background_thal: one run against one primer overran the work list");
    };
    if ((rc = run_slabs(ctx, {{0, (long)BackgroundSites::n_runs(total_len, k), 0, n}}, w.slabs, w.redone, nullptr, list,
                        [] {}, [](const Slab &, uint64_t, uint32_t &) { return MSSPE_OK; }, score, fold, cannot_split)))
        return rc;
    std::vector<uint64_t> host(4 * (size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), w.counts, sizeof(uint64_t) * host.size(), hipMemcpyDeviceToHost,
                                ctx->stream));
    if (keys) HIP_TRY(ctx, hipMemcpyAsync(&n_keys, aw.key_count, sizeof n_keys, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(host.begin(), host.begin() + 2 * (size_t)n, sites_out);
    std::copy(host.begin() + 2 * (size_t)n, host.end(), stable_out);
    if (keys) aw.n_keys = (long long)n_keys;
    w.flank_classes = __builtin_popcount(classes_seen);
    return MSSPE_OK;
}

// msspe_segment_coverage_thal*: the matches of the mm rule through the work list of msspe_background_thal*, slab by
// slab (groups [g0, g1) x primers [p0, p1)); a slab that overruns the list is split -- by groups while it has several,
// then by primers -- and listed again, and only a slab that fitted is scored and folded (run_slabs).
int coverage_thal_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                       const msspe_mismatch_opt *mm, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                       int n_rev, const msspe_chem *chem, int mode, float tm_threshold, uint8_t *held_out,
                       double *t_best_out, uint32_t *primer_segments_out, uint32_t *primer_held_out,
                       msspe_scored_match *matches, uint64_t capacity, uint64_t *count_out)
{
    if (!opt || !mm || !chem || !held_out || n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd_words) ||
        (n_rev && !rev_words) || (matches && !count_out))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (mode != 1 && mode != 2) return fail(ctx, MSSPE_ERR_ARG, "coverage_thal: mode must be 1 (ANY) or 2 (END1)");
    if (count_out) *count_out = 0;
    const int k = opt->kmer_size;
    if (k < 2 || k > 31) return fail(ctx, MSSPE_ERR_K, "coverage_thal: unsupported k (need 2 <= k <= 31)");
    std::string err;
    long P = 0;
    int rc = MismatchCoverage::check(n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p, fwd_words, n_fwd,
                                     rev_words, n_rev, &P, err);
    if (rc) return fail(ctx, rc, err);
    if (opt->search_window_size - k >= (1 << kCovOffBits))   // a match's offset travels in kCovOffBits bits
        return fail(ctx, MSSPE_ERR_ARG, "coverage_thal: the search window has more than 2^26 positions");
    const int n = n_fwd + n_rev;
    const long n_seg = P * n_seq;
    std::fill(held_out, held_out + n_seg, (uint8_t)0);
    if (t_best_out) std::fill(t_best_out, t_best_out + n_seg, 0.0);
    if (primer_segments_out) std::fill(primer_segments_out, primer_segments_out + n, 0u);
    if (primer_held_out) std::fill(primer_held_out, primer_held_out + n, 0u);
    auto &ct = ctx->cov_thal;
    ct.matches = ct.slabs = ct.redone = 0;
    ct.list_us = ct.score_us = ct.fold_us = 0;
    if (n == 0 || n_seg == 0) return MSSPE_OK;
    if (!site_pool_fits(ctx, n)) return fail(ctx, MSSPE_ERR_ARG, "coverage_thal: too many primers");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool end1 = mode == 2;
    ChemEntry *ce = nullptr;
    if ((rc = site_scoring_begin(ctx, *chem, tm_threshold, end1, k, 0, n, &ce))) return rc;
    const double cut = ce->c[0].g_cut;
    const size_t cap = site_list_cap(ctx);
    if ((rc = ct.prepare(*opt, fwd_words, n_fwd, rev_words, n_rev, n_seg, ctx->stream, err))) return fail(ctx, rc, err);
    auto &w = ctx->site_work;
    CovMatch *list = reinterpret_cast<CovMatch *>(w.sites);
    if ((rc = upload_site_pool(ctx, fwd_words, n_fwd, rev_words, n_rev))) return rc;
    msspe_scored_match *d_out = nullptr;
    uint64_t *d_count = nullptr;
    if (matches && (rc = ct.out_list(capacity, &d_out, &d_count, ctx->stream, err))) return fail(ctx, rc, err);

    const int S = MismatchCoverage::group_size(*opt);
    const long n_groups = (n_seg + S - 1) / S, chunk = CoverageThal::max_slab_groups(n);
    std::vector<Slab> todo;
    for (long g1 = n_groups; g1 > 0; g1 -= std::min(g1, chunk))   // popped from the back: ascending groups
        todo.push_back({g1 - std::min(g1, chunk), g1, 0, n});
    bool scored = false;   // ev[2..4] of a scored slab wait to be read behind the next synchronisation
    auto list_slab = [&](const Slab &s) -> int {
        HIP_TRY(ctx, hipEventRecord(ct.ev[0], ctx->stream));
        if ((rc = ct.list_slab(view, n_seg, P, *opt, mm->max_mismatches, mm->exact_3p, s.o0, s.o1, s.p0, s.p1, list,
                               cap, w.slab_count, ctx->stream, err)))
            return fail(ctx, rc, err);
        HIP_TRY(ctx, hipEventRecord(ct.ev[1], ctx->stream));
        return MSSPE_OK;
    };
    auto synced = [&] { read_slab_times(ct, true, scored); };
    auto prepare = [&](const Slab &, uint64_t, uint32_t &) -> int {
        HIP_TRY(ctx, hipEventRecord(ct.ev[2], ctx->stream));
        return MSSPE_OK;
    };
    auto score = [&](uint32_t c0, uint32_t cnt) -> int {
        HIP_TRY(ctx, ct.oligos(view, P, *opt, list, c0, cnt, w.pool, w.list + c0, ctx->ovf_count, ctx->stream));
        return score_site_pairs(ctx, ce, end1, n, k, k, w.list + c0, cnt);
    };
    auto fold = [&](const Slab &s, uint64_t count) -> int {
        HIP_TRY(ctx, hipEventRecord(ct.ev[3], ctx->stream));
        if ((rc = ct.fold_slab(list, (uint32_t)count, w.dg, w.t, cut, *opt, s.o0, s.o1, s.p0, s.p1, d_out, capacity,
                               d_count, ctx->stream, err)))
            return fail(ctx, rc, err);
        HIP_TRY(ctx, hipEventRecord(ct.ev[4], ctx->stream));
        scored = true;
        return MSSPE_OK;
    };
    auto cannot_split = [&](uint64_t count) {
        return fail(ctx, MSSPE_ERR_CAPACITY, site_list_overrun("coverage_thal", count, cap));
    };
    if ((rc = run_slabs(ctx, std::move(todo), ct.slabs, ct.redone, &ct.matches, list_slab, synced, prepare, score, fold,
                        cannot_split)))
        return rc;
    if ((rc = ct.finish(n_seg, held_out, t_best_out, primer_segments_out, primer_held_out, ctx->stream, err)))
        return fail(ctx, rc, err);
    read_slab_times(ct, false, scored);
    if (matches) {
        uint64_t count = 0;
        HIP_TRY(ctx, hipMemcpy(&count, d_count, sizeof count, hipMemcpyDeviceToHost));
        const uint64_t kept = std::min(count, capacity);
        if (kept) HIP_TRY(ctx, hipMemcpy(matches, d_out, sizeof(msspe_scored_match) * kept, hipMemcpyDeviceToHost));
        std::sort(matches, matches + kept, [](const msspe_scored_match &a, const msspe_scored_match &b) {
            if (a.primer != b.primer) return a.primer < b.primer;
            if (a.segment != b.segment) return a.segment < b.segment;
            return a.offset < b.offset;
        });
        *count_out = count;
        if (count > capacity) return fail(ctx, MSSPE_ERR_CAPACITY, "match list capacity too small");
    }
    return MSSPE_OK;
}

// The held incidence matrix of n_fwd + n_rev primers (msspe_panel_thin_thal*, and a tolerant seeded stage A's tiles):
// d_inc (PanelThin::matrix made it for them) zeroed, then the slab loop (run_slabs) into it.  The caller has
// the chemistry's entry, the workspace, the overflow lists, the work list for these primers, their plane words
// (CoverageThal::prepare_words) and the events; `scored` says that a last slab's ev[3..5] are still to be read
// (read_slab_times, behind the caller's next synchronisation).
int fill_held_matrix(msspe_ctx *ctx, const SeqView &view, long n_seg, long P, const msspe_kmer_opt *opt,
                     const msspe_mismatch_opt *mm, ChemEntry *ce, bool end1, const uint64_t *fwd_words, int n_fwd,
                     const uint64_t *rev_words, int n_rev, uint64_t *d_inc, bool &scored)
{
    auto &tt = ctx->thin_thal;
    auto &ct = ctx->cov_thal;
    std::string err;
    int rc;
    const int k = opt->kmer_size, n = n_fwd + n_rev;
    const size_t cap = site_list_cap(ctx);
    const double cut = ce->c[0].g_cut;
    const int S = MismatchCoverage::group_size(*opt);
    const long n_groups = (n_seg + S - 1) / S;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    HIP_TRY(ctx, hipMemsetAsync(d_inc, 0, sizeof(uint64_t) * (size_t)n_groups * n_pad, ctx->stream));
    auto &w = ctx->site_work;
    CovMatch *list = reinterpret_cast<CovMatch *>(w.sites);
    if ((rc = upload_site_pool(ctx, fwd_words, n_fwd, rev_words, n_rev))) return rc;
    const bool unique = ctx->opt.thin_thal_unique;

    auto list_slab = [&](const Slab &s) -> int {
        HIP_TRY(ctx, hipEventRecord(tt.ev[0], ctx->stream));
        if ((rc = ct.list_slab(view, n_seg, P, *opt, mm->max_mismatches, mm->exact_3p, s.o0, s.o1, s.p0, s.p1, list,
                               cap, w.slab_count, ctx->stream, err)))
            return fail(ctx, rc, err);
        HIP_TRY(ctx, hipEventRecord(tt.ev[1], ctx->stream));
        return MSSPE_OK;
    };
    auto synced = [&] { read_slab_times(tt, true, scored); };
    auto prepare = [&](const Slab &, uint64_t count, uint32_t &n_pairs) -> int {
        HIP_TRY(ctx, hipEventRecord(tt.ev[2], ctx->stream));
        if (unique) {
            // every template first, then the slab's runs: their pairs replace the identity pairs in w.list; the sort's
            // key planes are dg and t, which nothing reads before the scoring writes them
            HIP_TRY(ctx, ct.oligos(view, P, *opt, list, 0, (uint32_t)count, w.pool, w.list, ctx->ovf_count,
                                   ctx->stream));
            if ((rc = tt.unique(list, w.pool, n, k, (uint32_t)count, reinterpret_cast<uint64_t *>(w.dg),
                                reinterpret_cast<uint64_t *>(w.t), w.list, ctx->stream, err)))
                return fail(ctx, rc, err);
            HIP_TRY(ctx, hipEventRecord(tt.ev[3], ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(&n_pairs, tt.unique_count(), sizeof n_pairs, hipMemcpyDeviceToHost,
                                        ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (n_pairs == 0 || n_pairs > count)
                return fail(ctx, MSSPE_ERR_DEVICE, "panel thin thal: the distinct pairs of a slab do not add up");
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, tt.ev[2], tt.ev[3]) == hipSuccess) tt.unique_us += (long long)(ms * 1000.f);
        } else {
            HIP_TRY(ctx, hipEventRecord(tt.ev[3], ctx->stream));
        }
        tt.unique_pairs += n_pairs;
        return MSSPE_OK;
    };
    auto score = [&](uint32_t c0, uint32_t cnt) -> int {
        if (unique)   // the list's length, where oligos would have put it
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->ovf_count, (int)cnt, 1, ctx->stream));
        else
            HIP_TRY(ctx, ct.oligos(view, P, *opt, list, c0, cnt, w.pool, w.list + c0, ctx->ovf_count, ctx->stream));
        return score_site_pairs(ctx, ce, end1, n, k, k, w.list + c0, cnt);
    };
    auto fold = [&](const Slab &, uint64_t count) -> int {
        HIP_TRY(ctx, hipEventRecord(tt.ev[4], ctx->stream));
        if ((rc = tt.fold(list, (uint32_t)count, unique, w.t, cut, S, n_pad, d_inc, ctx->stream, err)))
            return fail(ctx, rc, err);
        HIP_TRY(ctx, hipEventRecord(tt.ev[5], ctx->stream));
        scored = true;
        return MSSPE_OK;
    };
    auto cannot_split = [&](uint64_t count) {
        return fail(ctx, MSSPE_ERR_CAPACITY, site_list_overrun("panel thin thal", count, cap));
    };
    return run_slabs(ctx, {{0, n_groups, 0, n}}, tt.slabs, tt.redone, &tt.matches, list_slab, synced, prepare, score,
                     fold, cannot_split);
}

// msspe_panel_thin_thal*: the slab loop (fill_held_matrix) into the held incidence matrix, then PanelThin::rounds over
// it.  No per-segment word, cell plane or record list is kept: a slab's matches are listed, their templates cut
// (CoverageThal::oligos), with thin_thal_unique the distinct (primer, template) pairs of the slab found
// (PanelThinThal::unique) and only those scored, and every stable match ORs its bit into the matrix, which is zeroed
// once: a slab split by groups or by primers adds to the words the others wrote.
int panel_thin_thal_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                         const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const msspe_chem *chem, int mode,
                         float tm_threshold, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                         int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                         int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                         long long *covered_kept_out, const msspe_thin_depth_opt *deep = nullptr,
                         uint8_t *depth_all_out = nullptr, uint8_t *depth_kept_out = nullptr,
                         long long *counts_out = nullptr)
{
    // deep: msspe_panel_thin_thal_depth* (thin is NULL then, and the three covered outputs are not used)
    if (!opt || !mm || (!thin && !deep) || !chem || !keep_out || !order_out || !gain_out || !n_picked_out || n_fwd < 0 ||
        n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: null argument");
    const int min_gain = deep ? deep->min_gain : thin->min_gain;
    if (min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: min_gain must be at least 1");
    if (deep && (deep->depth < 1 || deep->depth > 255))
        return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: depth must be 1..255");
    if (mode != 1 && mode != 2) return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: mode must be 1 (ANY) or 2 (END1)");
    auto &tt = ctx->thin_thal;
    tt.reset_stats();
    *n_picked_out = 0;
    if (covered_all_out) *covered_all_out = 0;
    if (covered_kept_out) *covered_kept_out = 0;
    if (counts_out) std::fill(counts_out, counts_out + 4, 0LL);
    const int k = opt->kmer_size;
    if (k < 2 || k > 31) return fail(ctx, MSSPE_ERR_K, "panel thin thal: unsupported k (need 2 <= k <= 31)");
    std::string err;
    long P = 0;
    int rc = MismatchCoverage::check(n_seq, seq_len, *opt, mm->max_mismatches, mm->exact_3p, fwd_words, n_fwd,
                                     rev_words, n_rev, &P, err);
    if (rc) return fail(ctx, rc, err);
    if (opt->search_window_size - k >= (1 << kCovOffBits))   // a match's offset travels in kCovOffBits bits
        return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: the search window has more than 2^26 positions");
    const int n = n_fwd + n_rev;
    const long n_seg = P * n_seq;
    for (int p = 0; p < n; ++p) keep_out[p] = forced && forced[p] ? 1 : 0;
    if (covered_out) std::fill(covered_out, covered_out + n_seg, (uint8_t)0);
    if (depth_all_out) std::fill(depth_all_out, depth_all_out + n_seg, (uint8_t)0);
    if (depth_kept_out) std::fill(depth_kept_out, depth_kept_out + n_seg, (uint8_t)0);
    if (n == 0 || n_seg == 0) return MSSPE_OK;
    if (!site_pool_fits(ctx, n)) return fail(ctx, MSSPE_ERR_ARG, "panel thin thal: too many primers");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool end1 = mode == 2;
    ChemEntry *ce = nullptr;
    if ((rc = site_scoring_begin(ctx, *chem, tm_threshold, end1, k, 0, n, &ce))) return rc;
    auto &ct = ctx->cov_thal;
    if ((rc = ct.prepare_words(*opt, fwd_words, n_fwd, rev_words, n_rev, ctx->stream, err))) return fail(ctx, rc, err);
    if ((rc = tt.events(err))) return fail(ctx, rc, err);
    const int S = MismatchCoverage::group_size(*opt);
    uint64_t *d_inc = nullptr;
    if ((rc = ctx->thin.matrix(n, n_seg, S, (size_t)ctx->opt.panel_thin_matrix_max_mb << 20, &d_inc, err)))
        return fail(ctx, rc, err);
    bool scored = false;
    if ((rc = fill_held_matrix(ctx, view, n_seg, P, opt, mm, ce, end1, fwd_words, n_fwd, rev_words, n_rev, d_inc, scored)))
        return rc;
    if (deep) {
        std::vector<uint8_t> shadow((size_t)n);
        (void)PanelThin::shadows(fwd_words, n_fwd, rev_words, n_rev, forced, shadow.data());
        rc = ctx->thin.rounds_depth(n, n_seg, S, min_gain, deep->depth, shadow.data(), keep_out, order_out, gain_out,
                                    n_picked_out, depth_all_out, depth_kept_out, counts_out, ctx->n_cu, ctx->stream,
                                    err);
    } else {
        rc = ctx->thin.rounds(n, n_seg, S, min_gain, keep_out, order_out, gain_out, n_picked_out, covered_out,
                              covered_all_out, covered_kept_out, ctx->n_cu, ctx->stream, err);
    }
    if (rc) return fail(ctx, rc, err);
    read_slab_times(ctx->thin_thal, false, scored);   // rounds returned with the stream idle
    return MSSPE_OK;
}

// msspe_panel_select*: the cover's graph over the pool "forward words then reverse words" (CoverStage::begin /
// prepare: one S in the context, whoever built it last), the thinning's matrix filled by the rule's mode (mode 0 as
// msspe_panel_thin*, modes 1 and 2 as msspe_panel_thin_thal*; a threshold <= 0 is mode 0), then PanelSelect::rounds.
// msspe_panel_select_depth*: the depth and the outputs the layered rule adds; the rest of such a call
// is the selection's, with covered_out, covered_all_out and covered_kept_out NULL.
struct SelectDepthArgs {
    int depth;
    uint8_t *pick_layer_out, *depth_all_out, *depth_kept_out;
    long long *counts_out;
};

int panel_select_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                      const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                      const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint64_t *d_bitmap,
                      uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                      uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                      long long *covered_kept_out, int *n_tubes_used_out, const SelectDepthArgs *dep = nullptr,
                      const PanelWeights *wts = nullptr, const PanelCosts *cst = nullptr)
{
    if (!opt || !rule || !sel || !keep_out || !order_out || !gain_out || !n_picked_out || !tube_out || n_fwd < 0 ||
        n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words))
        return fail(ctx, MSSPE_ERR_ARG, "panel select: null argument");
    if (sel->min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel select: min_gain must be at least 1");
    if (sel->max_tubes < 1 || sel->max_tubes > kTubeMax)
        return fail(ctx, MSSPE_ERR_ARG, "panel select: max_tubes must be 1..64");
    if (dep && (dep->depth < 1 || dep->depth > 255))
        return fail(ctx, MSSPE_ERR_ARG, "panel select: depth must be 1..255");
    if (rule->mode < 0 || rule->mode > 2)
        return fail(ctx, MSSPE_ERR_ARG, "panel select: mode must be 0, 1 (ANY) or 2 (END1)");
    if (rule->mode && !rule->chem) return fail(ctx, MSSPE_ERR_ARG, "panel select: modes 1 and 2 need a chemistry");
    ctx->select.reset_stats();
    ctx->select_prepare_us = ctx->select_incidence_us = 0;
    *n_picked_out = 0;
    if (covered_all_out) *covered_all_out = 0;
    if (covered_kept_out) *covered_kept_out = 0;
    if (n_tubes_used_out) *n_tubes_used_out = 0;
    if (dep && dep->counts_out) std::fill(dep->counts_out, dep->counts_out + 4, 0LL);
    const int k = opt->kmer_size;
    if (k < 2 || k > 31) return fail(ctx, MSSPE_ERR_K, "panel select: unsupported k (need 2 <= k <= 31)");
    if ((long)n_fwd + (long)n_rev > (long)kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "panel select: " + std::to_string((long)n_fwd + n_rev) + " primers, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    const int mode = rule->tm_threshold > 0.0f ? rule->mode : 0;   // a threshold <= 0: H is I
    const msspe_mismatch_opt mm = {rule->max_mismatches, rule->exact_3p};
    std::string err;
    long P = 0;
    int rc = MismatchCoverage::check(n_seq, seq_len, *opt, mm.max_mismatches, mm.exact_3p, fwd_words, n_fwd, rev_words,
                                     n_rev, &P, err);
    if (rc) return fail(ctx, rc, err);
    if (mode && opt->search_window_size - k >= (1 << kCovOffBits))   // a match's offset travels in kCovOffBits bits
        return fail(ctx, MSSPE_ERR_ARG, "panel select: the search window has more than 2^26 positions");
    if (wts)   // depth 1 only: no caller passes both
        if ((rc = panel_weights_check(ctx, "panel select", *wts, n_seq, seq_len, *opt, mm.max_mismatches, mm.exact_3p,
                                      fwd_words, n_fwd, rev_words, n_rev)))
            return rc;
    if (cst)   // depth 1 only, as the weights
        if ((rc = panel_costs_check(ctx, "panel select", *cst, n_fwd, n_rev))) return rc;
    const int n = n_fwd + n_rev;
    const long n_seg = P * n_seq;
    for (int p = 0; p < n; ++p) {
        keep_out[p] = forced && forced[p] ? 1 : 0;
        tube_out[p] = MSSPE_TUBE_NONE;
        if (barred_out) barred_out[p] = 0;
    }
    if (covered_out) std::fill(covered_out, covered_out + n_seg, (uint8_t)0);
    if (dep && dep->depth_all_out) std::fill(dep->depth_all_out, dep->depth_all_out + n_seg, (uint8_t)0);
    if (dep && dep->depth_kept_out) std::fill(dep->depth_kept_out, dep->depth_kept_out + n_seg, (uint8_t)0);
    if (n == 0 || n_seg == 0) return MSSPE_OK;
    if (!d_bitmap) return fail(ctx, MSSPE_ERR_ARG, "panel select: null bitmap");
    if (mode && !site_pool_fits(ctx, n)) return fail(ctx, MSSPE_ERR_ARG, "panel select: too many primers");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (auto &e : ctx->select_ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    const int S = MismatchCoverage::group_size(*opt);
    uint64_t *d_inc = nullptr;
    if ((rc = ctx->thin.matrix(n, n_seg, S, (size_t)ctx->opt.panel_thin_matrix_max_mb << 20, &d_inc, err)))
        return fail(ctx, rc, err);

    // the graph: S = B | B^T over the pool in the bitmap's order
    const uint64_t *d_pool = nullptr;
    if ((rc = ctx->select.begin(n, n_seg, S, fwd_words, n_fwd, rev_words, n_rev, &d_pool, ctx->stream, err)) ||
        (rc = ctx->cover.begin(n, k, ctx->stream, err)) ||
        (rc = ctx->cover.prepare(d_pool, n, k, d_bitmap, sel->drop_self_pairs != 0, ctx->stream, err)))
        return fail(ctx, rc, err);

    // the incidence
    HIP_TRY(ctx, hipEventRecord(ctx->select_ev[0], ctx->stream));
    bool scored = false;
    if (!mode) {
        if ((rc = ctx->mm_cov.incidence(view, n_seq, seq_len, *opt, mm.max_mismatches, mm.exact_3p, fwd_words, n_fwd,
                                        rev_words, n_rev, d_inc, ctx->stream, err)))
            return fail(ctx, rc, err);
    } else {
        auto &tt = ctx->thin_thal;
        tt.reset_stats();
        const bool end1 = mode == 2;
        ChemEntry *ce = nullptr;
        if ((rc = site_scoring_begin(ctx, *rule->chem, rule->tm_threshold, end1, k, 0, n, &ce))) return rc;
        if ((rc = ctx->cov_thal.prepare_words(*opt, fwd_words, n_fwd, rev_words, n_rev, ctx->stream, err)))
            return fail(ctx, rc, err);
        if ((rc = tt.events(err))) return fail(ctx, rc, err);
        if ((rc = fill_held_matrix(ctx, view, n_seg, P, opt, &mm, ce, end1, fwd_words, n_fwd, rev_words, n_rev, d_inc,
                                   scored)))
            return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->select_ev[1], ctx->stream));

    if (dep)
        rc = ctx->select.rounds_depth(d_inc, ctx->cover.symmetrised(), n, n_seg, S, sel->min_gain, sel->max_tubes,
                                      dep->depth, keep_out, order_out, gain_out, n_picked_out, tube_out, barred_out,
                                      n_tubes_used_out, dep->pick_layer_out, dep->depth_all_out, dep->depth_kept_out,
                                      dep->counts_out, ctx->n_cu, ctx->stream, err);
    else
        rc = ctx->select.rounds(d_inc, ctx->cover.symmetrised(), n, n_seg, S, sel->min_gain, sel->max_tubes, keep_out,
                                order_out, gain_out, n_picked_out, tube_out, barred_out, covered_out, covered_all_out,
                                covered_kept_out, n_tubes_used_out, ctx->n_cu, ctx->stream, err, wts, cst);
    if (rc) return fail(ctx, rc, err);
    read_slab_times(ctx->thin_thal, false, scored);   // rounds returned with the stream idle
    long long keys_us = 0, sym_us = 0;
    ctx->cover.prepare_us(keys_us, sym_us);
    ctx->select_prepare_us = keys_us + sym_us;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->select_ev[0], ctx->select_ev[1]) == hipSuccess)
        ctx->select_incidence_us = (long long)(ms * 1000.0f);
    return MSSPE_OK;
}

// ---- msspe_kmer_candidates_tolerant*: stage A seeded on what the panel covers --------------------------------------

// One direction of a tolerant call: its distinct seed words (msspe_pack_oligos form) and its two state outputs.
struct TolerantDir {
    std::vector<uint64_t> words;
    uint8_t *covered_out = nullptr;
    uint32_t *partitions_out = nullptr;
};

// The rule's own argument errors, and the coverage calls' for these options (MismatchCoverage::check over the seeds as
// the direction's primers; in modes 1 and 2 coverage_thal_view's); *P_out: partitions per record.
int tolerant_check(msspe_ctx *ctx, int n_seq, size_t seq_len, const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                   const msspe_kmer_sets *sets, int direction, long *P_out)
{
    if (rule->mode < 0 || rule->mode > 2) return fail(ctx, MSSPE_ERR_ARG, "tolerant seeding: mode must be 0, 1 (ANY) or 2 (END1)");
    if (rule->mode && !rule->chem) return fail(ctx, MSSPE_ERR_ARG, "tolerant seeding: modes 1 and 2 need a chemistry");
    const int k = opt->kmer_size;
    if (rule->mode && (k < 2 || k > 31)) return fail(ctx, MSSPE_ERR_K, "tolerant seeding: unsupported k (need 2 <= k <= 31)");
    const int ns = sets ? sets->n_seed : 0;
    const uint64_t *seed = sets ? sets->seed : nullptr;
    std::string err;
    const int rc = MismatchCoverage::check(n_seq, seq_len, *opt, rule->max_mismatches, rule->exact_3p, direction ? nullptr : seed,
                                           direction ? 0 : ns, direction ? seed : nullptr, direction ? ns : 0, P_out, err);
    if (rc) return fail(ctx, rc, err);
    if (rule->mode && opt->search_window_size - k >= (1 << kCovOffBits))
        return fail(ctx, MSSPE_ERR_ARG, "tolerant seeding: the search window has more than 2^26 positions");
    if (rule->mode && !site_pool_fits(ctx, ns))
        return fail(ctx, MSSPE_ERR_ARG, "tolerant seeding: too many seeds");
    return MSSPE_OK;
}

void tolerant_dir(const msspe_kmer_sets *sets, uint8_t *covered_out, uint32_t *partitions_out, long n_seg, long P,
                  TolerantDir &d)
{
    if (sets && sets->n_seed) d.words.assign(sets->seed, sets->seed + sets->n_seed);
    std::sort(d.words.begin(), d.words.end());
    d.words.erase(std::unique(d.words.begin(), d.words.end()), d.words.end());
    d.covered_out = covered_out;
    d.partitions_out = partitions_out;
    if (covered_out) std::fill(covered_out, covered_out + n_seg, (uint8_t)0);
    if (partitions_out) std::fill(partitions_out, partitions_out + P, 0u);
}

// What the seeding passes share and a second host thread must not make: the chemistry's entry, the DP workspace and
// the overflow lists of modes 1 and 2, the events.
int tolerant_prepare(msspe_ctx *ctx, const msspe_kmer_opt *opt, const msspe_seed_rule *rule, ChemEntry **ce_out)
{
    auto &tl = ctx->tolerant;
    tl.tiles = tl.segments = tl.incidence_us = tl.seed_us = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (auto &e : tl.ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    *ce_out = nullptr;
    if (!rule->mode) return MSSPE_OK;
    auto &tt = ctx->thin_thal;
    tt.reset_stats();
    int rc;
    if ((rc = site_scoring_begin(ctx, *rule->chem, rule->tm_threshold, rule->mode == 2, opt->kmer_size, 0, -1, ce_out)))
        return rc;
    std::string err;
    if ((rc = tt.events(err))) return fail(ctx, rc, err);
    return MSSPE_OK;
}

// One direction's seeding pass, called by KmerStage::run where k_seed would run.  The seeds go through the context's
// incidence matrix in tiles of primers, each against all segment groups -- the state is an OR (ignored) and a sum
// (coverage) over seeds, so the tiles add up -- sized so that a tile's matrix fits panel_thin_matrix_max_mb.  Mode 0
// fills a tile as msspe_panel_thin* does, modes 1 and 2 as msspe_panel_thin_thal* does; KmerStage::seed_rows turns
// its rows into the stage's state.  The pass runs on the context's stream, whichever stream the stage runs on (the
// matrix, the work list and the scoring are the context's), one pass at a time, and returns with both streams idle.
int tolerant_seed_pass(msspe_ctx *ctx, KmerStage &stage, hipStream_t stage_stream, const SeqView &view, int n_seq,
                       size_t seq_len, const msspe_kmer_opt *opt, int direction, const TolerantDir &d,
                       const msspe_seed_rule *rule, ChemEntry *ce, std::string &err)
{
    auto hip_bad = [&](hipError_t e, const char *what) {
        err = std::string("tolerant seeding, ") + what + ": " + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    };
#define TOL_TRY(expr)                                         \
    do {                                                      \
        hipError_t e__ = (expr);                              \
        if (e__ != hipSuccess) return hip_bad(e__, #expr);    \
    } while (0)
    if (stage_stream != ctx->stream) TOL_TRY(hipStreamSynchronize(stage_stream));   // the stage's state is set
    std::lock_guard<std::mutex> turn(ctx->tolerant.turn);
    auto &tl = ctx->tolerant;
    hipStream_t stream = ctx->stream;
    const msspe_mismatch_opt mm = {rule->max_mismatches, rule->exact_3p};
    const int n = (int)d.words.size();
    const long P = seq_len < (size_t)opt->segment_size
                       ? 0
                       : (long)((seq_len - (size_t)opt->segment_size) / (size_t)opt->overlap_size) + 1;
    const long n_seg = P * n_seq;
    const int S = MismatchCoverage::group_size(*opt);
    const long n_groups = (n_seg + S - 1) / S;
    const size_t mib = (size_t)1 << 20, max_bytes = (size_t)ctx->opt.panel_thin_matrix_max_mb << 20;
    const size_t fit = max_bytes / (sizeof(uint64_t) * (size_t)n_groups) & ~(size_t)63;   // seeds whose matrix fits
    if (fit < 64) {
        err = "tolerant seeding: the incidence matrix of 64 seeds needs " +
              std::to_string((64 * sizeof(uint64_t) * (size_t)n_groups + mib - 1) / mib) +
              " MB, panel_thin_matrix_max_mb is " + std::to_string(max_bytes / mib);
        return MSSPE_ERR_CAPACITY;
    }
    const int tile = (int)std::min<size_t>(fit, ((size_t)n + 63) & ~(size_t)63);
    int rc;
    if (rule->mode && (rc = ensure_site_work(ctx, site_list_cap(ctx), std::min(tile, n), 0))) {
        err = ctx->err;
        return rc;
    }
    for (int t0 = 0; t0 < n; t0 += tile) {
        const int nt = std::min(tile, n - t0);
        const size_t n_pad = ((size_t)nt + 63) & ~(size_t)63;
        const uint64_t *fwd = direction ? nullptr : d.words.data() + t0, *rev = direction ? d.words.data() + t0 : nullptr;
        const int n_fwd = direction ? 0 : nt, n_rev = direction ? nt : 0;
        uint64_t *d_inc = nullptr;
        if ((rc = ctx->thin.matrix(nt, n_seg, S, max_bytes, &d_inc, err))) return rc;
        TOL_TRY(hipEventRecord(tl.ev[0], stream));
        if (!rule->mode) {
            if ((rc = ctx->mm_cov.incidence(view, n_seq, seq_len, *opt, mm.max_mismatches, mm.exact_3p, fwd, n_fwd, rev,
                                            n_rev, d_inc, stream, err)))
                return rc;
        } else {
            if ((rc = ctx->cov_thal.prepare_words(*opt, fwd, n_fwd, rev, n_rev, stream, err))) return rc;
            bool scored = false;
            if ((rc = fill_held_matrix(ctx, view, n_seg, P, opt, &mm, ce, rule->mode == 2, fwd, n_fwd, rev, n_rev, d_inc,
                                       scored))) {
                err = ctx->err;
                return rc;
            }
            TOL_TRY(hipStreamSynchronize(stream));
            read_slab_times(ctx->thin_thal, false, scored);
        }
        TOL_TRY(hipEventRecord(tl.ev[1], stream));
        if ((rc = stage.seed_rows(d_inc, n_pad, nt, n_groups, S, stream, err))) return rc;
        TOL_TRY(hipEventRecord(tl.ev[2], stream));
        TOL_TRY(hipStreamSynchronize(stream));   // (the next tile's words and matrix take this one's place)
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, tl.ev[0], tl.ev[1]) == hipSuccess) tl.incidence_us += (long long)(a * 1000.f);
        if (hipEventElapsedTime(&b, tl.ev[1], tl.ev[2]) == hipSuccess) tl.seed_us += (long long)(b * 1000.f);
        ++tl.tiles;
    }
    long long covered = 0;
    if ((rc = stage.seed_state(d.covered_out, d.partitions_out, &covered, stage_stream, err))) return rc;
    tl.segments += covered;
    return MSSPE_OK;
#undef TOL_TRY
}

}  // namespace

// One direction of a tolerant call on the context's stream.  Without seeds it is the _sets call as it stands.
static int tolerant_run(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                        int direction, const msspe_kmer_sets *sets, const msspe_seed_rule *rule, uint64_t *words_out,
                        uint32_t *freq_out, int capacity, int *n_out, uint8_t *seed_covered_out,
                        uint32_t *seed_partitions_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if ((!view.ascii && !view.packed) || !opt || !rule || !words_out || !freq_out || !n_out || capacity < 0 ||
        !sets_ok(sets))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    *n_out = 0;
    if (direction != 0 && direction != 1) return fail(ctx, MSSPE_ERR_ARG, "tolerant seeding: direction must be 0 or 1");
    long P = 0;
    int rc = tolerant_check(ctx, n_seq, seq_len, opt, rule, sets, direction, &P);
    if (rc) return rc;
    TolerantDir d;
    tolerant_dir(sets, seed_covered_out, seed_partitions_out, P * n_seq, P, d);
    if (d.words.empty()) {
        auto &tl = ctx->tolerant;
        tl.tiles = tl.segments = tl.incidence_us = tl.seed_us = 0;
        return kmer_run(ctx, view, n_seq, seq_len, opt, direction, sets, words_out, freq_out, capacity, n_out);
    }
    ChemEntry *ce = nullptr;
    if ((rc = tolerant_prepare(ctx, opt, rule, &ce))) return rc;
    const KmerStage::SeedFrom seed_from = [&](KmerStage &stage, hipStream_t stream, std::string &err) {
        return tolerant_seed_pass(ctx, stage, stream, view, n_seq, seq_len, opt, direction, d, rule, ce, err);
    };
    const msspe_kmer_sets excl = {nullptr, 0, sets->exclude, sets->n_exclude};
    return kmer_run(ctx, view, n_seq, seq_len, opt, direction, &excl, words_out, freq_out, capacity, n_out, &seed_from);
}

int msspe_kmer_candidates_tolerant_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                              const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                              const msspe_seed_rule *rule, uint64_t *words_out, uint32_t *freq_out,
                                              int capacity, int *n_out, uint8_t *seed_covered_out,
                                              uint32_t *seed_partitions_out)
{
    return tolerant_run(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, direction, sets, rule, words_out,
                        freq_out, capacity, n_out, seed_covered_out, seed_partitions_out);
}

int msspe_kmer_candidates_tolerant(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                   const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                   const msspe_seed_rule *rule, uint64_t *words_out, uint32_t *freq_out, int capacity,
                                   int *n_out, uint8_t *seed_covered_out, uint32_t *seed_partitions_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!sets_ok(sets)) return fail(ctx, MSSPE_ERR_ARG, "null seed or exclusion list");
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = tolerant_run(ctx, SeqView{(const uint8_t *)d, nullptr, seq_len}, n_seq, seq_len, opt, direction, sets, rule,
                      words_out, freq_out, capacity, n_out, seed_covered_out, seed_partitions_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_kmer_candidates_both_tolerant_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                                   const msspe_kmer_opt *opt, const msspe_kmer_sets *fwd,
                                                   const msspe_kmer_sets *rev, const msspe_seed_rule *rule,
                                                   uint64_t *words_fwd, uint32_t *freq_fwd, int *n_fwd,
                                                   uint64_t *words_rev, uint32_t *freq_rev, int *n_rev, int capacity,
                                                   uint8_t *seed_covered_fwd, uint32_t *seed_partitions_fwd,
                                                   uint8_t *seed_covered_rev, uint32_t *seed_partitions_rev)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed || !opt || !rule || !words_fwd || !freq_fwd || !n_fwd || !words_rev || !freq_rev || !n_rev ||
        capacity < 0 || !sets_ok(fwd) || !sets_ok(rev))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    *n_fwd = *n_rev = 0;
    long P = 0;
    int rc;
    if ((rc = tolerant_check(ctx, n_seq, seq_len, opt, rule, fwd, 0, &P)) ||
        (rc = tolerant_check(ctx, n_seq, seq_len, opt, rule, rev, 1, &P)))
        return rc;
    TolerantDir d[2];
    tolerant_dir(fwd, seed_covered_fwd, seed_partitions_fwd, P * n_seq, P, d[0]);
    tolerant_dir(rev, seed_covered_rev, seed_partitions_rev, P * n_seq, P, d[1]);
    ChemEntry *ce = nullptr;
    auto &tl = ctx->tolerant;
    tl.tiles = tl.segments = tl.incidence_us = tl.seed_us = 0;
    if ((!d[0].words.empty() || !d[1].words.empty()) && (rc = tolerant_prepare(ctx, opt, rule, &ce))) return rc;
    const SeqView view{nullptr, d_packed, seq_len};
    // a direction without seeds runs as the _sets call does; the other's pass takes the context's stream in its turn
    const KmerStage::SeedFrom from_fwd = [&](KmerStage &stage, hipStream_t stream, std::string &err) {
        return tolerant_seed_pass(ctx, stage, stream, view, n_seq, seq_len, opt, 0, d[0], rule, ce, err);
    };
    const KmerStage::SeedFrom from_rev = [&](KmerStage &stage, hipStream_t stream, std::string &err) {
        return tolerant_seed_pass(ctx, stage, stream, view, n_seq, seq_len, opt, 1, d[1], rule, ce, err);
    };
    const msspe_kmer_sets excl_fwd = {nullptr, 0, fwd ? fwd->exclude : nullptr, fwd ? fwd->n_exclude : 0};
    const msspe_kmer_sets excl_rev = {nullptr, 0, rev ? rev->exclude : nullptr, rev ? rev->n_exclude : 0};
    return kmer_run_both(ctx, d_packed, n_seq, seq_len, opt, d[0].words.empty() ? fwd : &excl_fwd,
                         d[1].words.empty() ? rev : &excl_rev, words_fwd, freq_fwd, n_fwd, words_rev, freq_rev, n_rev,
                         capacity, d[0].words.empty() ? nullptr : &from_fwd, d[1].words.empty() ? nullptr : &from_rev);
}

int msspe_segment_coverage_thal_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const uint64_t *fwd_words,
                                    int n_fwd, const uint64_t *rev_words, int n_rev, const msspe_chem *chem, int mode,
                                    float tm_threshold, uint8_t *held_out, double *t_best_out,
                                    uint32_t *primer_segments_out, uint32_t *primer_held_out,
                                    msspe_scored_match *matches, uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return coverage_thal_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, fwd_words, n_fwd,
                              rev_words, n_rev, chem, mode, tm_threshold, held_out, t_best_out, primer_segments_out,
                              primer_held_out, matches, capacity, count_out);
}

int msspe_segment_coverage_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                           const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                           const msspe_chem *chem, int mode, float tm_threshold, uint8_t *held_out,
                                           double *t_best_out, uint32_t *primer_segments_out,
                                           uint32_t *primer_held_out, msspe_scored_match *matches, uint64_t capacity,
                                           uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return coverage_thal_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, fwd_words, n_fwd,
                              rev_words, n_rev, chem, mode, tm_threshold, held_out, t_best_out, primer_segments_out,
                              primer_held_out, matches, capacity, count_out);
}

int msspe_segment_coverage_thal(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const uint64_t *fwd_words,
                                int n_fwd, const uint64_t *rev_words, int n_rev, const msspe_chem *chem, int mode,
                                float tm_threshold, uint8_t *held_out, double *t_best_out,
                                uint32_t *primer_segments_out, uint32_t *primer_held_out, msspe_scored_match *matches,
                                uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_segment_coverage_thal_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, fwd_words, n_fwd,
                                         rev_words, n_rev, chem, mode, tm_threshold, held_out, t_best_out,
                                         primer_segments_out, primer_held_out, matches, capacity, count_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_panel_thin_thal_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                              const msspe_chem *chem, int mode, float tm_threshold, const uint64_t *fwd_words,
                              int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                              uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                              uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_thal_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, thin, chem, mode,
                                tm_threshold, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out,
                                n_picked_out, covered_out, covered_all_out, covered_kept_out);
}

int msspe_panel_thin_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                     const msspe_thin_opt *thin, const msspe_chem *chem, int mode, float tm_threshold,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                     int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                                     long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_thal_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, thin, chem, mode,
                                tm_threshold, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out,
                                n_picked_out, covered_out, covered_all_out, covered_kept_out);
}

int msspe_panel_thin_thal(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                          const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const msspe_chem *chem, int mode,
                          float tm_threshold, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                          int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                          int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                          long long *covered_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_thal_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, chem, mode, tm_threshold,
                                   fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out,
                                   n_picked_out, covered_out, covered_all_out, covered_kept_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_panel_thin_thal_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                    const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode,
                                    float tm_threshold, const uint64_t *fwd_words, int n_fwd,
                                    const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                                    uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_thal_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, mm, nullptr, chem, mode,
                                tm_threshold, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out,
                                n_picked_out, nullptr, nullptr, nullptr, thin, depth_all_out, depth_kept_out,
                                counts_out);
}

int msspe_panel_thin_thal_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                           const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode,
                                           float tm_threshold, const uint64_t *fwd_words, int n_fwd,
                                           const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                           uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                           int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                           long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_thin_thal_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, mm, nullptr, chem, mode,
                                tm_threshold, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out, gain_out,
                                n_picked_out, nullptr, nullptr, nullptr, thin, depth_all_out, depth_kept_out,
                                counts_out);
}

int msspe_panel_thin_thal_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode, float tm_threshold,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    rc = msspe_panel_thin_thal_depth_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, mm, thin, chem, mode,
                                         tm_threshold, fwd_words, n_fwd, rev_words, n_rev, forced, keep_out, order_out,
                                         gain_out, n_picked_out, depth_all_out, depth_kept_out, counts_out);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_panel_select_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                           const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words,
                           int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                           const uint64_t *d_bitmap, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                           int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                           long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_select_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd,
                             rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, covered_out, covered_all_out, covered_kept_out, n_tubes_used_out);
}

int msspe_panel_select_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  const uint8_t *forced, const uint64_t *d_bitmap, uint8_t *keep_out,
                                  uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                                  uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                                  long long *covered_kept_out, int *n_tubes_used_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_select_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd,
                             rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, covered_out, covered_all_out, covered_kept_out, n_tubes_used_out);
}

// The host forms: the alignment and the graph go to the device for the call (chem == NULL: `bitmap` is the graph,
// from the host; otherwise the pool is screened there, under conflict_rule where there is one, else under dg_threshold),
// the rest is msspe_panel_select_dev.
static int panel_select_host(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                             const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words,
                             int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                             const uint64_t *bitmap, const msspe_chem *chem, float dg_threshold, uint8_t *keep_out,
                             uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                             uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                             long long *covered_kept_out, int *n_tubes_used_out,
                             const msspe_conflict_rule *conflict_rule = nullptr, const SelectDepthArgs *dep = nullptr,
                             const PanelWeights *wts = nullptr, const PanelCosts *cst = nullptr)
{
    if (!seqs || n_seq < 0) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    if (n_fwd < 0 || n_rev < 0 || (n_fwd && !fwd_words) || (n_rev && !rev_words) || !opt || !rule || !sel || !keep_out ||
        !order_out || !gain_out || !n_picked_out || !tube_out)
        return fail(ctx, MSSPE_ERR_ARG, "panel select: null argument");
    if (sel->min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel select: min_gain must be at least 1");
    if (sel->max_tubes < 1 || sel->max_tubes > kTubeMax)   // before the screen, not after it
        return fail(ctx, MSSPE_ERR_ARG, "panel select: max_tubes must be 1..64");
    if (dep && (dep->depth < 1 || dep->depth > 255))
        return fail(ctx, MSSPE_ERR_ARG, "panel select: depth must be 1..255");
    const long n = (long)n_fwd + (long)n_rev;
    if (n > (long)kCoverMaxN)
        return fail(ctx, MSSPE_ERR_ARG, "panel select: " + std::to_string(n) + " primers, at most " +
                                            std::to_string(kCoverMaxN) + " (the symmetrised bitmap is n^2 / 8 bytes)");
    const int k = opt->kmer_size;
    if (k < 2 || k > 31) return fail(ctx, MSSPE_ERR_K, "panel select: unsupported k (need 2 <= k <= 31)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t words = ((size_t)n + 63) / 64;
    DevBuf<uint64_t> d_pool, d_bitmap;
    if (n) {
        HIP_TRY(ctx, d_bitmap.alloc((size_t)n * words));
        if (chem) {
            std::vector<uint64_t> pool(fwd_words, fwd_words + n_fwd);
            pool.insert(pool.end(), rev_words, rev_words + n_rev);
            for (uint64_t w : pool)   // the screen reads k bases of a word and nothing above them
                if (k < 32 && (w >> (2 * k))) return fail(ctx, MSSPE_ERR_ARG, "panel select: a primer word has bits above 2 k");
            {   // duplicates before the screen, not after it
                std::vector<uint64_t> s(pool);
                std::sort(s.begin(), s.end());
                if (std::adjacent_find(s.begin(), s.end()) != s.end())
                    return fail(ctx, MSSPE_ERR_ARG, "panel select: the primer lists hold duplicate words");
            }
            HIP_TRY(ctx, d_pool.alloc((size_t)n));
            HIP_TRY(ctx, hipMemcpyAsync(d_pool, pool.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice,
                                        ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pool leaves scope
            // the screen's decisions only: the bitmap is all the selection reads
            if (int rc = consumer_screen(ctx, d_pool, (int)n, k, chem, conflict_rule, dg_threshold, d_bitmap)) return rc;
        } else {
            if (!bitmap) return fail(ctx, MSSPE_ERR_ARG, "panel select: null bitmap");
            HIP_TRY(ctx, hipMemcpy(d_bitmap, bitmap, sizeof(uint64_t) * (size_t)n * words, hipMemcpyHostToDevice));
        }
    }
    void *d = nullptr;
    int rc = msspe_device_put(ctx, seqs, (size_t)n_seq * seq_len, &d);
    if (rc) return rc;
    if (dep)
        rc = panel_select_view(ctx, SeqView{(const uint8_t *)d, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel,
                               fwd_words, n_fwd, rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out,
                               n_picked_out, tube_out, barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, dep);
    else if (wts || cst)
        rc = panel_select_view(ctx, SeqView{(const uint8_t *)d, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel,
                               fwd_words, n_fwd, rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out,
                               n_picked_out, tube_out, barred_out, covered_out, covered_all_out, covered_kept_out,
                               n_tubes_used_out, nullptr, wts, cst);
    else
        rc = msspe_panel_select_dev(ctx, (const uint8_t *)d, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd,
                                    rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out,
                                    tube_out, barred_out, covered_out, covered_all_out, covered_kept_out,
                                    n_tubes_used_out);
    if (!rc && chem && n) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        rc = e != hipSuccess ? hip_fail(ctx, e, "hipStreamSynchronize") : check_list_overrun(ctx);
    }
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_panel_select(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                       const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                       const uint64_t *rev_words, int n_rev, const uint8_t *forced, const msspe_chem *chem,
                       float dg_threshold, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                       int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                       long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!chem) return fail(ctx, MSSPE_ERR_ARG, "panel select: null chemistry");
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev, forced,
                             nullptr, chem, dg_threshold, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, covered_out, covered_all_out, covered_kept_out, n_tubes_used_out);
}

int msspe_panel_select_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                            const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words,
                            int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                            const msspe_chem *chem, const msspe_conflict_rule *conflict_rule, uint8_t *keep_out,
                            uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                            uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                            long long *covered_kept_out, int *n_tubes_used_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, conflict_rule, GraphOut{}, false)) return rc;
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev, forced,
                             nullptr, chem, 0.0f, keep_out, order_out, gain_out, n_picked_out, tube_out, barred_out,
                             covered_out, covered_all_out, covered_kept_out, n_tubes_used_out, conflict_rule);
}

// msspe_panel_select_weighted*: the selection with a weight per segment; the rest of such a call is
// its unweighted sibling's.
int msspe_panel_select_weighted_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                    const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                    const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights,
                                    uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                    long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                    uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    return panel_select_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd,
                             rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, covered_out, covered_all_out, covered_kept_out, n_tubes_used_out, nullptr,
                             &wts);
}

int msspe_panel_select_weighted_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                           const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                           const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                           const uint64_t *d_bitmap, const uint32_t *weights, uint8_t *keep_out,
                                           uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                           uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                           long long *covered_all_out, long long *covered_kept_out,
                                           int *n_tubes_used_out, uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    return panel_select_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd,
                             rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, covered_out, covered_all_out, covered_kept_out, n_tubes_used_out, nullptr,
                             &wts);
}

int msspe_panel_select_weighted_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, const msspe_chem *chem,
                                     const msspe_conflict_rule *conflict_rule, const uint32_t *weights,
                                     uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                     uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                     long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                     uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, conflict_rule, GraphOut{}, false)) return rc;
    if (weight_all_out) *weight_all_out = 0;
    if (weight_kept_out) *weight_kept_out = 0;
    if (!weights)   // before the screen, not after it
        return fail(ctx, MSSPE_ERR_ARG, "panel select: null weights (the unweighted call takes none)");
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev, forced,
                             nullptr, chem, 0.0f, keep_out, order_out, gain_out, n_picked_out, tube_out, barred_out,
                             covered_out, covered_all_out, covered_kept_out, n_tubes_used_out, conflict_rule, nullptr,
                             &wts);
}

// msspe_panel_select_cost*: the selection by gain per cost; the rest of such a call is its sibling's,
// weighted or not.  Without weights the two weight sums are the two covered counts.
static void cost_counts_out(const uint32_t *weights, long long all, long long kept, long long *covered_all_out,
                            long long *covered_kept_out, uint64_t *weight_all_out, uint64_t *weight_kept_out)
{
    if (covered_all_out) *covered_all_out = all;
    if (covered_kept_out) *covered_kept_out = kept;
    if (!weights) {
        if (weight_all_out) *weight_all_out = (uint64_t)all;
        if (weight_kept_out) *weight_kept_out = (uint64_t)kept;
    }
}

static int panel_select_cost_view(msspe_ctx *ctx, const SeqView &view, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights, const uint32_t *costs,
                                  uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                  uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                  long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                  uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                  uint64_t *cost_kept_out)
{
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    const PanelCosts cst = {costs, cost_all_out, cost_kept_out};
    long long all = 0, kept = 0;
    const int rc = panel_select_view(ctx, view, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev,
                                     forced, d_bitmap, keep_out, order_out, gain_out, n_picked_out, tube_out, barred_out,
                                     covered_out, &all, &kept, n_tubes_used_out, nullptr, weights ? &wts : nullptr,
                                     &cst);
    cost_counts_out(weights, all, kept, covered_all_out, covered_kept_out, weight_all_out, weight_kept_out);
    return rc;
}

int msspe_panel_select_cost_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights, const uint32_t *costs,
                                uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_select_cost_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words,
                                  n_fwd, rev_words, n_rev, forced, d_bitmap, weights, costs, keep_out, order_out,
                                  gain_out, n_picked_out, tube_out, barred_out, covered_out, covered_all_out,
                                  covered_kept_out, n_tubes_used_out, weight_all_out, weight_kept_out, cost_all_out,
                                  cost_kept_out);
}

int msspe_panel_select_cost_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                       const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                       const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                       const uint64_t *rev_words, int n_rev,
                                       const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights, const uint32_t *costs,
                                       uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                       uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                       long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                       uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                       uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    return panel_select_cost_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, rule, sel, fwd_words,
                                  n_fwd, rev_words, n_rev, forced, d_bitmap, weights, costs, keep_out, order_out,
                                  gain_out, n_picked_out, tube_out, barred_out, covered_out, covered_all_out,
                                  covered_kept_out, n_tubes_used_out, weight_all_out, weight_kept_out, cost_all_out,
                                  cost_kept_out);
}

int msspe_panel_select_cost_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                 const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                 const uint8_t *forced, const msspe_chem *chem,
                                 const msspe_conflict_rule *conflict_rule, const uint32_t *weights,
                                 const uint32_t *costs, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                 int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                 long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                 uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                 uint64_t *cost_kept_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, conflict_rule, GraphOut{}, false)) return rc;
    if (weight_all_out) *weight_all_out = 0;
    if (weight_kept_out) *weight_kept_out = 0;
    const PanelWeights wts = {weights, weight_all_out, weight_kept_out};
    const PanelCosts cst = {costs, cost_all_out, cost_kept_out};
    if (n_fwd < 0 || n_rev < 0) return fail(ctx, MSSPE_ERR_ARG, "panel select: null argument");
    if (int rc = panel_costs_check(ctx, "panel select", cst, n_fwd, n_rev)) return rc;   // before the screen, not after it
    long long all = 0, kept = 0;
    const int rc = panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev,
                                     forced, nullptr, chem, 0.0f, keep_out, order_out, gain_out, n_picked_out, tube_out,
                                     barred_out, covered_out, &all, &kept, n_tubes_used_out, conflict_rule, nullptr,
                                     weights ? &wts : nullptr, &cst);
    cost_counts_out(weights, all, kept, covered_all_out, covered_kept_out, weight_all_out, weight_kept_out);
    return rc;
}

int msspe_panel_select_bitmap(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              const uint8_t *forced, const uint64_t *bitmap, uint8_t *keep_out, uint32_t *order_out,
                              uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                              uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
                              int *n_tubes_used_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel, fwd_words, n_fwd, rev_words, n_rev, forced,
                             bitmap, nullptr, 0.0f, keep_out, order_out, gain_out, n_picked_out, tube_out, barred_out,
                             covered_out, covered_all_out, covered_kept_out, n_tubes_used_out);
}

// msspe_panel_select_depth*: the five forms of the selection with the depth behind the options.  A NULL sel is the
// selection's error (the view and the host form name it).
#define SELECT_DEPTH_ARGS                                                                              \
    const msspe_select_opt so = {sel ? sel->min_gain : 0, sel ? sel->max_tubes : 0, sel ? sel->drop_self_pairs : 0}; \
    const SelectDepthArgs dep = {sel ? sel->depth : 1, pick_layer_out, depth_all_out, depth_kept_out, counts_out}

int msspe_panel_select_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                 const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                 const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint64_t *d_bitmap,
                                 uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                 uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out,
                                 uint8_t *pick_layer_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                 long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_seqs) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    SELECT_DEPTH_ARGS;
    return panel_select_view(ctx, SeqView{d_seqs, nullptr, seq_len}, n_seq, seq_len, opt, rule, sel ? &so : nullptr,
                             fwd_words, n_fwd, rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out,
                             n_picked_out, tube_out, barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, &dep);
}

int msspe_panel_select_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                        const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                        const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                        const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                        const uint64_t *d_bitmap, uint8_t *keep_out, uint32_t *order_out,
                                        uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                                        int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                                        uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!d_packed) return fail(ctx, MSSPE_ERR_ARG, "null sequences");
    SELECT_DEPTH_ARGS;
    return panel_select_view(ctx, SeqView{nullptr, d_packed, seq_len}, n_seq, seq_len, opt, rule, sel ? &so : nullptr,
                             fwd_words, n_fwd, rev_words, n_rev, forced, d_bitmap, keep_out, order_out, gain_out,
                             n_picked_out, tube_out, barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, &dep);
}

int msspe_panel_select_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                             const msspe_seed_rule *rule, const msspe_select_depth_opt *sel, const uint64_t *fwd_words,
                             int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                             const msspe_chem *chem, float dg_threshold, uint8_t *keep_out, uint32_t *order_out,
                             uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                             int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                             uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!chem) return fail(ctx, MSSPE_ERR_ARG, "panel select: null chemistry");
    SELECT_DEPTH_ARGS;
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel ? &so : nullptr, fwd_words, n_fwd, rev_words,
                             n_rev, forced, nullptr, chem, dg_threshold, keep_out, order_out, gain_out, n_picked_out,
                             tube_out, barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, nullptr, &dep);
}

int msspe_panel_select_depth_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                  const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                  const uint64_t *rev_words, int n_rev, const uint8_t *forced, const msspe_chem *chem,
                                  const msspe_conflict_rule *conflict_rule, uint8_t *keep_out, uint32_t *order_out,
                                  uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                                  int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                                  uint8_t *depth_kept_out, long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (int rc = graph_rule_check(ctx, chem, conflict_rule, GraphOut{}, false)) return rc;
    SELECT_DEPTH_ARGS;
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel ? &so : nullptr, fwd_words, n_fwd, rev_words,
                             n_rev, forced, nullptr, chem, 0.0f, keep_out, order_out, gain_out, n_picked_out, tube_out,
                             barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, conflict_rule, &dep);
}

int msspe_panel_select_depth_bitmap(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                    const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                    const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint64_t *bitmap,
                                    uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out,
                                    uint8_t *pick_layer_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                    long long *counts_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    SELECT_DEPTH_ARGS;
    return panel_select_host(ctx, seqs, n_seq, seq_len, opt, rule, sel ? &so : nullptr, fwd_words, n_fwd, rev_words,
                             n_rev, forced, bitmap, nullptr, 0.0f, keep_out, order_out, gain_out, n_picked_out,
                             tube_out, barred_out, nullptr, nullptr, nullptr, n_tubes_used_out, nullptr, &dep);
}
#undef SELECT_DEPTH_ARGS

int msspe_background_thal_flank_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                           const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                           const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                           uint64_t *sites_out, uint64_t *stable_out, msspe_scored_site *d_sites,
                                           uint64_t capacity, uint64_t *d_count)
{
    return background_thal_pass(ctx, d_packed, total_len, k, mm, words, n, chem, mode, tm_threshold, flank, sites_out,
                                stable_out, d_sites, capacity, d_count, false);
}

int msspe_background_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                     const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                     const msspe_chem *chem, int mode, float tm_threshold, uint64_t *sites_out,
                                     uint64_t *stable_out, msspe_scored_site *d_sites, uint64_t capacity,
                                     uint64_t *d_count)
{
    return msspe_background_thal_flank_packed_dev(ctx, d_packed, total_len, k, mm, words, n, chem, mode, tm_threshold,
                                                  0, sites_out, stable_out, d_sites, capacity, d_count);
}

int msspe_background_thal(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                          int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                          int mode, float tm_threshold, uint64_t *sites_out, uint64_t *stable_out,
                          msspe_scored_site *sites, uint64_t capacity, uint64_t *count_out,
                          uint64_t *record_start_out)
{
    return msspe_background_thal_flank(ctx, records, record_bytes, n_records, k, mm, words, n, chem, mode,
                                       tm_threshold, 0, sites_out, stable_out, sites, capacity, count_out,
                                       record_start_out);
}

int msspe_background_thal_flank(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                int n_records, int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                const msspe_chem *chem, int mode, float tm_threshold, int flank, uint64_t *sites_out,
                                uint64_t *stable_out, msspe_scored_site *sites, uint64_t capacity,
                                uint64_t *count_out, uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!mm || !sites_out || !stable_out || !chem || n < 0 || (n && !words) || (sites && !count_out))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (count_out) *count_out = 0;
    void *d = nullptr;
    size_t L = 0;
    int rc = msspe_device_put_stream_packed(ctx, records, record_bytes, n_records, &d, &L, record_start_out);
    if (rc) return rc;
    msspe_scored_site *d_sites = nullptr;   // the list and, behind it, its count
    uint64_t *d_count = nullptr;
    hipError_t e = hipSuccess;
    if (sites) {
        const size_t list_bytes = sizeof(msspe_scored_site) * (size_t)capacity;
        e = hipMalloc((void **)&d_sites, list_bytes + sizeof(uint64_t));
        if (e == hipSuccess) {
            d_count = (uint64_t *)((char *)d_sites + list_bytes);
            e = hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream);
        }
    }
    if (e == hipSuccess) {
        rc = msspe_background_thal_flank_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode,
                                                    tm_threshold, flank, sites_out, stable_out, d_sites, capacity,
                                                    d_count);
        if (!rc && sites) {
            uint64_t count = 0;
            e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            const uint64_t kept = std::min(count, capacity);
            if (e == hipSuccess && kept)
                e = hipMemcpy(sites, d_sites, sizeof(msspe_scored_site) * kept, hipMemcpyDeviceToHost);
            if (e == hipSuccess) {
                std::sort(sites, sites + kept, [](const msspe_scored_site &a, const msspe_scored_site &b) {
                    if (a.primer != b.primer) return a.primer < b.primer;
                    if (a.strand != b.strand) return a.strand < b.strand;
                    return a.pos < b.pos;
                });
                *count_out = count;
                if (count > capacity) rc = fail(ctx, MSSPE_ERR_CAPACITY, "site list capacity too small");
            }
        }
    }
    if (d_sites) (void)hipFree(d_sites);
    (void)msspe_device_free(ctx, d);
    if (e != hipSuccess) return hip_fail(ctx, e, "msspe_background_thal");
    return rc;
}

int msspe_background_amplicons_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                          const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                          const msspe_chem *chem, int mode, float tm_threshold,
                                          const msspe_amplicon_opt *amp, const uint64_t *record_start, int n_records,
                                          uint64_t *sites_out, uint64_t *stable_out, uint64_t *amplicons_out,
                                          uint64_t *n_amplicons_out, msspe_amplicon *d_amplicons, uint64_t capacity,
                                          uint64_t *d_count)
{
    return msspe_background_amplicons_flank_packed_dev(ctx, d_packed, total_len, k, mm, words, n, chem, mode,
                                                       tm_threshold, 0, amp, record_start, n_records, sites_out,
                                                       stable_out, amplicons_out, n_amplicons_out, d_amplicons,
                                                       capacity, d_count);
}

int msspe_background_amplicons_flank_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                                const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                                const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                                const msspe_amplicon_opt *amp, const uint64_t *record_start,
                                                int n_records, uint64_t *sites_out, uint64_t *stable_out,
                                                uint64_t *amplicons_out, uint64_t *n_amplicons_out,
                                                msspe_amplicon *d_amplicons, uint64_t capacity, uint64_t *d_count)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!amp || !amplicons_out || !n_amplicons_out || n < 0 || (d_amplicons && !d_count) ||
        (record_start && n_records <= 0))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (k >= 2 && k <= 31 && amp->min_len < (uint32_t)k)   // another k: the scored pass's MSSPE_ERR_K
        return fail(ctx, MSSPE_ERR_ARG, "background_amplicons: min_len is shorter than the primers");
    if (amp->min_len > amp->max_len) return fail(ctx, MSSPE_ERR_ARG, "background_amplicons: min_len exceeds max_len");
    if (record_start) {
        if (record_start[0] != 0)
            return fail(ctx, MSSPE_ERR_ARG, "background_amplicons: record_start[0] must be 0");
        for (int r = 1; r < n_records; ++r)
            if (record_start[r] <= record_start[r - 1])
                return fail(ctx, MSSPE_ERR_ARG, "background_amplicons: record_start is not ascending");
        if (record_start[n_records - 1] > total_len)
            return fail(ctx, MSSPE_ERR_ARG, "background_amplicons: a record starts beyond the stream");
    }
    *n_amplicons_out = 0;
    int rc = background_thal_pass(ctx, d_packed, total_len, k, mm, words, n, chem, mode, tm_threshold, flank,
                                  sites_out, stable_out, nullptr, 0, nullptr, true);
    if (rc) return rc;
    std::fill(amplicons_out, amplicons_out + 2 * (size_t)n, (uint64_t)0);
    auto &w = ctx->amp_work;
    w.sort_us = w.join_us = 0;
    const uint64_t m = (uint64_t)w.n_keys;
    if (!m) return MSSPE_OK;
    if (m >= (1ull << 31)) return fail(ctx, MSSPE_ERR_NOMEM, "background_amplicons: 2^31 stable sites or more");
    unsigned end_bit = 33;   // position bits above the strand and the primer
    while (end_bit < 64 && (total_len >> (end_bit - 32))) ++end_bit;
    const size_t tmp_bytes = amplicon_sort_temp_bytes((size_t)m, end_bit);
    if (w.sorted_cap < m) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.sorted) (void)hipFree(w.sorted);
        if (w.rec) (void)hipFree(w.rec);
        w.sorted = nullptr;
        w.rec = nullptr;
        w.sorted_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.sorted, sizeof(uint64_t) * m));
        HIP_TRY(ctx, hipMalloc((void **)&w.rec, sizeof(uint32_t) * m));
        w.sorted_cap = m;
    }
    if (w.tmp_bytes < tmp_bytes) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.tmp) (void)hipFree(w.tmp);
        w.tmp = nullptr;
        w.tmp_bytes = 0;
        HIP_TRY(ctx, hipMalloc(&w.tmp, tmp_bytes));
        w.tmp_bytes = tmp_bytes;
    }
    if (w.counts_cap < 2 * (size_t)n) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.counts) (void)hipFree(w.counts);
        w.counts = nullptr;
        w.counts_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.counts, sizeof(uint64_t) * 2 * (size_t)n));
        w.counts_cap = 2 * (size_t)n;
    }
    if (record_start && w.starts_cap < (size_t)n_records) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.starts) (void)hipFree(w.starts);
        w.starts = nullptr;
        w.starts_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.starts, sizeof(uint64_t) * (size_t)n_records));
        w.starts_cap = (size_t)n_records;
    }
    for (hipEvent_t &e : w.ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    HIP_TRY(ctx, hipMemsetAsync(w.counts, 0, sizeof(uint64_t) * 2 * (size_t)n, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[0], ctx->stream));
    HIP_TRY(ctx, sort_amplicon_keys(w.keys, w.sorted, (size_t)m, end_bit, w.tmp, w.tmp_bytes, ctx->stream));
    if (record_start) {
        // the call returns behind a synchronisation of the stream, so the caller's array outlives the copy
        HIP_TRY(ctx, hipMemcpyAsync(w.starts, record_start, sizeof(uint64_t) * (size_t)n_records,
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, launch_key_records(w.sorted, (uint32_t)m, w.starts, n_records, w.rec, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemsetAsync(w.rec, 0, sizeof(uint32_t) * m, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(w.ev[1], ctx->stream));
    HIP_TRY(ctx, launch_amplicon_join(w.sorted, w.rec, (uint32_t)m, k, amp->min_len, amp->max_len, w.counts,
                                      d_amplicons, capacity, d_amplicons ? d_count : nullptr, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[2], ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(amplicons_out, w.counts, sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    w.sort_us = (long long)(ms * 1000.0f);
    HIP_TRY(ctx, hipEventElapsedTime(&ms, w.ev[1], w.ev[2]));
    w.join_us = (long long)(ms * 1000.0f);
    uint64_t total = 0;
    for (int i = 0; i < n; ++i) total += amplicons_out[2 * (size_t)i];   // every amplicon has one forward primer
    *n_amplicons_out = total;
    return MSSPE_OK;
}

int msspe_background_amplicons(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                               int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                               const msspe_chem *chem, int mode, float tm_threshold, const msspe_amplicon_opt *amp,
                               uint64_t *sites_out, uint64_t *stable_out, uint64_t *amplicons_out,
                               uint64_t *n_amplicons_out, msspe_amplicon *amplicons, uint64_t capacity,
                               uint64_t *count_out, uint64_t *record_start_out)
{
    return msspe_background_amplicons_flank(ctx, records, record_bytes, n_records, k, mm, words, n, chem, mode,
                                            tm_threshold, 0, amp, sites_out, stable_out, amplicons_out,
                                            n_amplicons_out, amplicons, capacity, count_out, record_start_out);
}

int msspe_background_amplicons_flank(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                     int n_records, int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                     const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                     const msspe_amplicon_opt *amp, uint64_t *sites_out, uint64_t *stable_out,
                                     uint64_t *amplicons_out, uint64_t *n_amplicons_out, msspe_amplicon *amplicons,
                                     uint64_t capacity, uint64_t *count_out, uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!mm || !sites_out || !stable_out || !chem || !amp || !amplicons_out || !n_amplicons_out || n < 0 ||
        (n && !words) || (amplicons && !count_out))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (count_out) *count_out = 0;
    *n_amplicons_out = 0;
    void *d = nullptr;
    size_t L = 0;
    std::vector<uint64_t> starts((size_t)std::max(n_records, 0));
    int rc = msspe_device_put_stream_packed(ctx, records, record_bytes, n_records, &d, &L, starts.data());
    if (rc) return rc;
    if (record_start_out) std::copy(starts.begin(), starts.end(), record_start_out);
    msspe_amplicon *d_list = nullptr;   // the list and, behind it, its count
    uint64_t *d_count = nullptr;
    hipError_t e = hipSuccess;
    if (amplicons) {
        const size_t list_bytes = sizeof(msspe_amplicon) * (size_t)capacity;
        e = hipMalloc((void **)&d_list, list_bytes + sizeof(uint64_t));
        if (e == hipSuccess) {
            d_count = (uint64_t *)((char *)d_list + list_bytes);
            e = hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream);
        }
    }
    if (e == hipSuccess) {
        rc = msspe_background_amplicons_flank_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode,
                                                         tm_threshold, flank, amp,
                                                         n_records > 0 ? starts.data() : nullptr, n_records, sites_out,
                                                         stable_out, amplicons_out, n_amplicons_out, d_list, capacity,
                                                         d_count);
        if (!rc && amplicons) {
            uint64_t count = 0;
            e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            const uint64_t kept = std::min(count, capacity);
            if (e == hipSuccess && kept)
                e = hipMemcpy(amplicons, d_list, sizeof(msspe_amplicon) * kept, hipMemcpyDeviceToHost);
            if (e == hipSuccess) {
                std::sort(amplicons, amplicons + kept, [](const msspe_amplicon &a, const msspe_amplicon &b) {
                    if (a.pos != b.pos) return a.pos < b.pos;
                    if (a.len != b.len) return a.len < b.len;
                    if (a.fwd != b.fwd) return a.fwd < b.fwd;
                    return a.rev < b.rev;
                });
                *count_out = count;
                if (count > capacity) rc = fail(ctx, MSSPE_ERR_CAPACITY, "amplicon list capacity too small");
            }
        }
    }
    if (d_list) (void)hipFree(d_list);
    (void)msspe_device_free(ctx, d);
    if (e != hipSuccess) return hip_fail(ctx, e, "msspe_background_amplicons");
    return rc;
}

// Work buffers of msspe_stream_reach*: grown when a call needs more, kept otherwise.
static int ensure_reach_work(msspe_ctx *ctx, size_t total_len, int n_records)
{
    auto &w = ctx->reach_work;
    w.grows = 0;
    const size_t nw = std::max<size_t>(reach_plane_words(total_len), 1), nt = std::max<size_t>(reach_tiles(total_len), 1);
    if (w.plane_words < nw) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.planes) (void)hipFree(w.planes);
        w.planes = nullptr;
        w.plane_words = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.planes, 3 * sizeof(uint64_t) * nw));
        w.plane_words = nw;
        ++w.grows;
    }
    if (w.tiles_cap < nt) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.tiles) (void)hipFree(w.tiles);
        w.tiles = nullptr;
        w.tiles_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.tiles, 3 * sizeof(uint32_t) * nt));
        w.tiles_cap = nt;
    }
    if (w.records_cap < (size_t)n_records) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (w.starts) (void)hipFree(w.starts);
        if (w.acc) (void)hipFree(w.acc);
        w.starts = nullptr;
        w.acc = nullptr;
        w.records_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&w.starts, sizeof(uint64_t) * (size_t)n_records));
        HIP_TRY(ctx, hipMalloc((void **)&w.acc, sizeof(ReachAccum) * (size_t)n_records));
        w.records_cap = (size_t)n_records;
    }
    for (hipEvent_t &e : w.ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    return MSSPE_OK;
}

// From the two site planes of ctx->reach_work (ensure_reach_work) to one msspe_reach_record per record: the six launches
// behind the scored pass.  starts: HOST, nr entries.
static int reach_report(msspe_ctx *ctx, size_t total_len, int k, uint32_t reach, const uint64_t *starts, int nr,
                        msspe_reach_record *records_out)
{
    auto &w = ctx->reach_work;
    uint64_t *plus = w.planes, *minus = plus + w.plane_words, *neither = minus + w.plane_words;
    const size_t nt = reach_tiles(total_len);
    uint32_t *tile_plus = w.tiles, *tile_minus = tile_plus + w.tiles_cap, *tile_zero = tile_minus + w.tiles_cap;
    // the call returns behind a synchronisation of the stream, so the caller's array outlives the copy
    HIP_TRY(ctx, hipMemcpyAsync(w.starts, starts, sizeof(uint64_t) * (size_t)nr, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w.acc, 0, sizeof(ReachAccum) * (size_t)nr, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[0], ctx->stream));
    HIP_TRY(ctx, launch_reach_tiles(plus, minus, total_len, k, tile_plus, tile_minus, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[1], ctx->stream));
    HIP_TRY(ctx, launch_reach_scan(tile_plus, tile_minus, nt, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[2], ctx->stream));
    HIP_TRY(ctx, launch_reach_masks(plus, minus, total_len, k, reach, w.starts, nr, tile_plus, tile_minus,
                                    w.acc, neither, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[3], ctx->stream));
    HIP_TRY(ctx, launch_reach_gap_tiles(neither, total_len, tile_zero, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[4], ctx->stream));
    HIP_TRY(ctx, launch_reach_scan(tile_zero, nullptr, nt, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[5], ctx->stream));
    HIP_TRY(ctx, launch_reach_gaps(neither, total_len, w.starts, nr, tile_zero, w.acc, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(w.ev[6], ctx->stream));
    std::vector<ReachAccum> host((size_t)nr);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), w.acc, sizeof(ReachAccum) * host.size(), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 6; ++i) {
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, w.ev[i], w.ev[i + 1]));
        w.us[i] = (long long)(ms * 1000.0f);
    }
    for (int r = 0; r < nr; ++r) {
        const ReachAccum &a = host[(size_t)r];
        const uint32_t s = (uint32_t)starts[r];
        auto len = [](unsigned long long key) { return (uint32_t)(key >> 32); };
        auto pos = [&](unsigned long long key) { return key >> 32 ? ~(uint32_t)key : s; };
        records_out[r] = msspe_reach_record{a.sites_plus,    a.sites_minus,     a.reached_plus,   a.reached_minus,
                                            a.reached_either, a.reached_both,    len(a.gap_plus),  pos(a.gap_plus),
                                            len(a.gap_minus), pos(a.gap_minus),  len(a.gap_either), pos(a.gap_either)};
    }
    return MSSPE_OK;
}

int msspe_stream_reach_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                  const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                                  int mode, float tm_threshold, int flank, const msspe_reach_opt *reach_opt,
                                  const uint64_t *record_start, int n_records, uint64_t *sites_out,
                                  uint64_t *stable_out, msspe_reach_record *records_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!reach_opt || !records_out || (record_start && n_records <= 0))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (k >= 2 && k <= 31 && reach_opt->reach < (uint32_t)k)   // another k: the scored pass's MSSPE_ERR_K
        return fail(ctx, MSSPE_ERR_ARG, "stream_reach: reach is shorter than the primers");
    if (reach_opt->reach >= (1u << 31)) return fail(ctx, MSSPE_ERR_ARG, "stream_reach: reach must be below 2^31");
    if (record_start) {
        if (record_start[0] != 0) return fail(ctx, MSSPE_ERR_ARG, "stream_reach: record_start[0] must be 0");
        for (int r = 1; r < n_records; ++r)
            if (record_start[r] <= record_start[r - 1])
                return fail(ctx, MSSPE_ERR_ARG, "stream_reach: record_start is not ascending");
        if (record_start[n_records - 1] > total_len)
            return fail(ctx, MSSPE_ERR_ARG, "stream_reach: a record starts beyond the stream");
    }
    const uint64_t one_start = 0;
    const uint64_t *starts = record_start ? record_start : &one_start;
    const int nr = record_start ? n_records : 1;
    auto end_of = [&](int r) { return r + 1 < nr ? starts[r + 1] - 1 : (uint64_t)total_len; };
    auto &w = ctx->reach_work;
    for (long long &u : w.us) u = 0;
    w.grows = 0;
    const bool empty = n == 0 || total_len < (size_t)k;   // the scored pass returns before it touches the device
    uint64_t *plus = nullptr, *minus = nullptr;
    if (!empty && total_len < ((size_t)1 << 32) && d_packed && mm && chem && sites_out && stable_out && n > 0 &&
        words && k >= 2 && k <= 31) {   // anything else: the scored pass names the fault
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (int rc = ensure_reach_work(ctx, total_len, nr)) return rc;
        plus = w.planes;
        minus = plus + w.plane_words;
        HIP_TRY(ctx, hipMemsetAsync(plus, 0, 2 * sizeof(uint64_t) * w.plane_words, ctx->stream));
    }
    int rc = background_thal_pass(ctx, d_packed, total_len, k, mm, words, n, chem, mode, tm_threshold, flank,
                                  sites_out, stable_out, nullptr, 0, nullptr, false, plus, minus);
    if (rc) return rc;
    if (empty) {   // no site: nothing is reached and every gap is its whole record
        for (int r = 0; r < nr; ++r) {
            const uint32_t s = (uint32_t)starts[r], len = (uint32_t)(end_of(r) - starts[r]);
            records_out[r] = msspe_reach_record{0, 0, 0, 0, 0, 0, len, s, len, s, len, s};
        }
        return MSSPE_OK;
    }
    if (!plus) return fail(ctx, MSSPE_ERR_ARG, "stream_reach: unsupported arguments");
    return reach_report(ctx, total_len, k, reach_opt->reach, starts, nr, records_out);
}

int msspe_stream_reach(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records, int k,
                       const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem, int mode,
                       float tm_threshold, int flank, const msspe_reach_opt *reach_opt, uint64_t *sites_out,
                       uint64_t *stable_out, msspe_reach_record *records_out, uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!mm || !sites_out || !stable_out || !chem || !reach_opt || !records_out || n < 0 || (n && !words))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    void *d = nullptr;
    size_t L = 0;
    std::vector<uint64_t> starts((size_t)std::max(n_records, 0));
    int rc = msspe_device_put_stream_packed(ctx, records, record_bytes, n_records, &d, &L, starts.data());
    if (rc) return rc;
    if (record_start_out) std::copy(starts.begin(), starts.end(), record_start_out);
    if (n_records > 0)
        rc = msspe_stream_reach_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode, tm_threshold,
                                           flank, reach_opt, starts.data(), n_records, sites_out, stable_out,
                                           records_out);
    else {   // no record: nothing to report on, but the arguments are still checked
        msspe_reach_record none;
        rc = msspe_stream_reach_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode, tm_threshold,
                                           flank, reach_opt, nullptr, 0, sites_out, stable_out, &none);
    }
    (void)msspe_device_free(ctx, d);
    return rc;
}

// msspe_panel_thin_reach*: the scored pass in its keys mode, the cover over columns (panel_thin_reach.hip) on the
// "neither" plane of reach_work, then the reach report from the kept primers' keys -- no second scored pass.
int msspe_panel_thin_reach_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                      const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                      const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                      const msspe_reach_opt *reach_opt, const msspe_thin_opt *thin,
                                      const uint8_t *forced, const uint64_t *record_start, int n_records,
                                      uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                      uint32_t *reach_out, long long *reached_all_out, long long *reached_kept_out,
                                      uint64_t *sites_out, uint64_t *stable_out, msspe_reach_record *records_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!reach_opt || !thin || !keep_out || !order_out || !gain_out || !n_picked_out || n < 0 ||
        (record_start && n_records <= 0))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    if (thin->min_gain < 1) return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: min_gain must be at least 1");
    if (k >= 2 && k <= 31 && reach_opt->reach < (uint32_t)k)   // another k: the scored pass's MSSPE_ERR_K
        return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: reach is shorter than the primers");
    if (reach_opt->reach >= (1u << 31)) return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: reach must be below 2^31");
    if (record_start) {
        if (record_start[0] != 0) return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: record_start[0] must be 0");
        for (int r = 1; r < n_records; ++r)
            if (record_start[r] <= record_start[r - 1])
                return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: record_start is not ascending");
        if (record_start[n_records - 1] > total_len)
            return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: a record starts beyond the stream");
    }
    const uint64_t one_start = 0;
    const uint64_t *starts = record_start ? record_start : &one_start;
    const int nr = record_start ? n_records : 1;
    auto end_of = [&](int r) { return r + 1 < nr ? starts[r + 1] - 1 : (uint64_t)total_len; };
    *n_picked_out = 0;
    if (reached_all_out) *reached_all_out = 0;
    if (reached_kept_out) *reached_kept_out = 0;
    ctx->thin_reach.reset();
    auto &w = ctx->reach_work;
    for (long long &u : w.us) u = 0;
    w.grows = 0;
    int rc = background_thal_pass(ctx, d_packed, total_len, k, mm, words, n, chem, mode, tm_threshold, flank,
                                  sites_out, stable_out, nullptr, 0, nullptr, true);
    if (rc) return rc;
    for (int p = 0; p < n; ++p) keep_out[p] = forced && forced[p] ? 1 : 0;
    if (reach_out) std::fill(reach_out, reach_out + n, 0u);
    if (n == 0 || total_len < (size_t)k) {   // the scored pass returned before it touched the device
        for (int r = 0; records_out && r < nr; ++r) {
            const uint32_t s = (uint32_t)starts[r], len = (uint32_t)(end_of(r) - starts[r]);
            records_out[r] = msspe_reach_record{0, 0, 0, 0, 0, 0, len, s, len, s, len, s};
        }
        return MSSPE_OK;
    }
    if (total_len >= ((size_t)1 << 32)) return fail(ctx, MSSPE_ERR_ARG, "panel_thin_reach: unsupported arguments");
    const uint64_t m = (uint64_t)ctx->amp_work.n_keys;
    if (m >= (1ull << 31)) return fail(ctx, MSSPE_ERR_NOMEM, "panel_thin_reach: 2^31 stable sites or more");
    if ((rc = ensure_reach_work(ctx, total_len, nr))) return rc;
    uint64_t *plus = w.planes, *minus = plus + w.plane_words, *neither = minus + w.plane_words;
    HIP_TRY(ctx, hipMemcpyAsync(w.starts, starts, sizeof(uint64_t) * (size_t)nr, hipMemcpyHostToDevice, ctx->stream));
    if (records_out) HIP_TRY(ctx, hipMemsetAsync(plus, 0, 2 * sizeof(uint64_t) * w.plane_words, ctx->stream));
    std::string err;
    if ((rc = ctx->thin_reach.run(ctx->amp_work.keys, (uint32_t)m, n, total_len, k, reach_opt->reach, w.starts, nr,
                                  neither, records_out ? plus : nullptr, records_out ? minus : nullptr,
                                  (uint32_t)thin->min_gain, keep_out, order_out, gain_out, n_picked_out, reach_out,
                                  reached_all_out, reached_kept_out, ctx->stream, err)))
        return fail(ctx, rc, err);
    if (records_out && (rc = reach_report(ctx, total_len, k, reach_opt->reach, starts, nr, records_out))) return rc;
    if ((rc = ctx->thin_reach.end_report(ctx->stream, err))) return fail(ctx, rc, err);
    return MSSPE_OK;
}

int msspe_panel_thin_reach(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                           int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                           int mode, float tm_threshold, int flank, const msspe_reach_opt *reach_opt,
                           const msspe_thin_opt *thin, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out,
                           uint32_t *gain_out, int *n_picked_out, uint32_t *reach_out, long long *reached_all_out,
                           long long *reached_kept_out, uint64_t *sites_out, uint64_t *stable_out,
                           msspe_reach_record *records_out, uint64_t *record_start_out)
{
    if (!ctx) return MSSPE_ERR_ARG;
    if (!mm || !sites_out || !stable_out || !chem || !reach_opt || !thin || !keep_out || !order_out || !gain_out ||
        !n_picked_out || n < 0 || (n && !words))
        return fail(ctx, MSSPE_ERR_ARG, "null argument");
    void *d = nullptr;
    size_t L = 0;
    std::vector<uint64_t> starts((size_t)std::max(n_records, 0));
    int rc = msspe_device_put_stream_packed(ctx, records, record_bytes, n_records, &d, &L, starts.data());
    if (rc) return rc;
    if (record_start_out) std::copy(starts.begin(), starts.end(), record_start_out);
    if (n_records > 0)
        rc = msspe_panel_thin_reach_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode, tm_threshold,
                                               flank, reach_opt, thin, forced, starts.data(), n_records, keep_out,
                                               order_out, gain_out, n_picked_out, reach_out, reached_all_out,
                                               reached_kept_out, sites_out, stable_out, records_out);
    else   // no record: nothing to report on, but the arguments are still checked
        rc = msspe_panel_thin_reach_packed_dev(ctx, (const uint64_t *)d, L, k, mm, words, n, chem, mode, tm_threshold,
                                               flank, reach_opt, thin, forced, nullptr, 0, keep_out, order_out,
                                               gain_out, n_picked_out, reach_out, reached_all_out, reached_kept_out,
                                               sites_out, stable_out, nullptr);
    (void)msspe_device_free(ctx, d);
    return rc;
}

int msspe_host_pair_tables(const char *params_path, const msspe_chem *chem, float dg_threshold,
                           double *fast_S, int32_t *fast_H, int32_t *int_g, int32_t *int_T,
                           double consts[8])
{
    // host only (no device needed): what the all-pairs kernels keep in LDS, for the CPU tests
    if (!chem || !fast_S || !fast_H || !int_g || !int_T || !consts) return MSSPE_ERR_ARG;
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                           chem->max_loop, false, dg_threshold);
    auto pt = std::make_unique<PairTables>();
    if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_ERR_TABLES;
    auto ft = std::make_unique<FastTables>();
    auto it = std::make_unique<IntTables>();
    const bool fast_ok = build_fast_tables(*tb, *pt, pairs_fast_max_k(), *ft);
    const bool int_ok = fast_ok && build_int_tables(*ft, pairs_fast_max_k(), *it);
    std::memcpy(fast_S, ft->S, sizeof ft->S);
    std::memcpy(fast_H, ft->H, sizeof ft->H);
    std::memcpy(int_g, it->g, sizeof it->g);
    std::memcpy(int_T, it->T, sizeof it->T);
    consts[0] = c.init_S;
    consts[1] = c.RC;
    consts[2] = c.salt;
    consts[3] = c.temp_k;
    consts[4] = c.g_cut;
    consts[5] = fast_ok ? 1.0 : 0.0;
    consts[6] = int_ok ? 1.0 : 0.0;
    consts[7] = (double)FastTables::kCount;
    return MSSPE_OK;
}

int msspe_host_table_routes(const char *params_path, const msspe_chem *chem, int32_t out[8])
{
    // host only: the flags chem_entry() would set for these tables and this chemistry
    if (!chem || !out) return MSSPE_ERR_ARG;
    for (int q = 0; q < 8; ++q) out[q] = 0;
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    if (!(chem->dna_conc > 0) || chem->max_loop < 0 || chem->max_loop > 30) return MSSPE_ERR_ARG;
    auto pt = std::make_unique<PairTables>();
    for (int sym = 1; sym >= 0; --sym) {   // the ordinary tables last: they are the ones the routes are built from
        const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                               chem->max_loop, sym == 1, -9000.0f);
        if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_OK;   // out[0] = 0: every dimer call is refused
    }
    auto ft = std::make_unique<FastTables>();
    auto it = std::make_unique<IntTables>();
    auto st = std::make_unique<SplitTables>();
    const TableRoutes r = table_routes(*tb, *pt, chem->max_loop, *ft, *it, *st);
    out[0] = 1;
    out[1] = r.fast_ok;
    out[2] = r.int_ok;
    out[3] = r.row_ok;
    out[4] = r.split_max_k > 0;
    out[5] = r.split_max_k;
    out[6] = r.wave_max_k;
    return MSSPE_OK;
}

int msspe_host_screen_plan(int first_stage, int row0, int row1, int col0, int ncols, int64_t list_cap, int64_t *out,
                           int capacity, int *n_out)
{
    // host only: the first-stage launches run_chain issues for this block under hand-over lists of list_cap entries
    if (!n_out || capacity < 0 || (capacity > 0 && !out)) return MSSPE_ERR_ARG;
    *n_out = 0;
    if (first_stage < 0 || first_stage > (int)FirstStage::BoundMirror || row0 < 0 || row1 <= row0 || col0 < 0 || ncols < 1 ||
        (long)col0 + ncols > (long)INT32_MAX || list_cap < 1)
        return MSSPE_ERR_ARG;
    const FirstStage first = (FirstStage)first_stage;
    if (first == FirstStage::BoundMirror && (row0 != col0 || row1 - row0 != ncols || ncols > mirror_launch_cap((long)list_cap)))
        return MSSPE_ERR_ARG;   // settle_first_stage's conditions on the block
    ScreenPlan plan;
    try {
        plan = plan_screen(first, row0, row1, col0, ncols, (long)list_cap);
    } catch (const std::bad_alloc &) {
        return MSSPE_ERR_NOMEM;
    }
    if (plan.launches.size() > (size_t)INT32_MAX) return MSSPE_ERR_NOMEM;
    *n_out = (int)plan.launches.size();
    if (*n_out > capacity) return MSSPE_ERR_CAPACITY;
    for (const Launch &l : plan.launches) {
        const int64_t row[7] = {l.row0, l.row1, l.col0, l.col1, l.pairs, l.list_entries, l.flush_before ? 1 : 0};
        out = std::copy(row, row + 7, out);
    }
    return MSSPE_OK;
}

int msspe_host_slab_split(int64_t o0, int64_t o1, int p0, int p1, uint64_t count, uint64_t cap, int64_t *out,
                          int capacity, int *n_out)
{
    // host only: the parts run_slabs lists again for a slab whose `count` matches overran a work list of `cap`
    if (!n_out || capacity < 0 || (capacity > 0 && !out)) return MSSPE_ERR_ARG;
    *n_out = 0;
    if (o0 < 0 || o1 <= o0 || o1 - o0 > INT32_MAX || p0 < 0 || p1 <= p0 || cap < 1 || count <= cap ||
        count > (UINT64_MAX - cap) / 2)   // (the last two: what the rule's 64-bit arithmetic holds)
        return MSSPE_ERR_ARG;
    std::vector<Slab> parts;
    try {
        (void)split_slab({(long)o0, (long)o1, p0, p1}, count, cap, parts);   // no parts: the slab cannot be split
    } catch (const std::bad_alloc &) {
        return MSSPE_ERR_NOMEM;
    }
    *n_out = (int)parts.size();
    if (*n_out > capacity) return MSSPE_ERR_CAPACITY;
    for (const Slab &s : parts) {
        const int64_t row[4] = {s.o0, s.o1, s.p0, s.p1};
        out = std::copy(row, row + 4, out);
    }
    return MSSPE_OK;
}

int msspe_host_bound_tables(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *bound_g,
                            int32_t *bound_T, int32_t info[8])
{
    // host only: the bound first stage's tables (csrc/fast_tables.hpp BoundTables) as chem_entry() would build them
    if (!chem || !bound_g || !bound_T || !info) return MSSPE_ERR_ARG;
    for (int q = 0; q < 8; ++q) info[q] = 0;
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    if (!(chem->dna_conc > 0) || chem->max_loop < 0 || chem->max_loop > 30) return MSSPE_ERR_ARG;
    const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                           chem->max_loop, false, dg_threshold);
    auto pt = std::make_unique<PairTables>();
    if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_ERR_TABLES;
    auto ft = std::make_unique<FastTables>();
    auto it = std::make_unique<IntTables>();
    auto st = std::make_unique<SplitTables>();
    const TableRoutes r = table_routes(*tb, *pt, chem->max_loop, *ft, *it, *st);
    auto bt = std::make_unique<BoundTables>();
    const bool ok = build_bound_tables(*ft, c, pairs_bound_max_k(), *bt) && r.row_ok;
    std::memcpy(bound_g, bt->g, sizeof bt->g);
    std::memcpy(bound_T, bt->T, sizeof bt->T);
    info[0] = ok ? 1 : 0;
    info[1] = bt->init;
    info[2] = bt->cut;
    info[3] = BoundTables::kUnitInv;
    info[4] = BoundTables::kMargin;
    info[5] = BoundTables::kReach;
    info[6] = IntTables::kValid;
    info[7] = pairs_bound_max_k();
    return MSSPE_OK;
}

// host only: the packed bound instance's tables (csrc/fast_tables.hpp BoundPacked) as chem_entry() would build them;
// all zero where the instance does not apply
static int host_bound_packed(const char *params_path, const msspe_chem *chem, float dg_threshold, BoundPacked &out)
{
    std::memset(&out, 0, sizeof out);
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    if (!(chem->dna_conc > 0) || chem->max_loop < 0 || chem->max_loop > 30) return MSSPE_ERR_ARG;
    const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                           chem->max_loop, false, dg_threshold);
    auto pt = std::make_unique<PairTables>();
    if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_ERR_TABLES;
    auto ft = std::make_unique<FastTables>();
    auto it = std::make_unique<IntTables>();
    auto st = std::make_unique<SplitTables>();
    const TableRoutes r = table_routes(*tb, *pt, chem->max_loop, *ft, *it, *st);
    auto bt = std::make_unique<BoundTables>();
    const bool ok = build_bound_tables(*ft, c, pairs_bound_max_k(), *bt) && r.row_ok &&
                    build_bound_packed(*bt, pairs_bound_max_k(), out);
    if (!ok) std::memset(&out, 0, sizeof out);
    return MSSPE_OK;
}

int msspe_host_bound_packed(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *packed_g,
                            int32_t *packed_T, int32_t info[8])
{
    if (!chem || !packed_g || !packed_T || !info) return MSSPE_ERR_ARG;
    for (int q = 0; q < 8; ++q) info[q] = 0;
    auto bp = std::make_unique<BoundPacked>();
    if (int rc = host_bound_packed(params_path, chem, dg_threshold, *bp)) return rc;
    const bool ok = bp->usable != 0;
    std::memcpy(packed_g, bp->q.g, sizeof bp->q.g);
    std::memcpy(packed_T, bp->q.T, sizeof bp->q.T);
    info[0] = ok ? 1 : 0;
    info[1] = bp->shift;
    info[2] = bp->bias;
    info[3] = bp->lo;
    info[4] = bp->hi;
    info[5] = bp->q.init;
    info[6] = bp->q.cut;
    info[7] = BoundPacked::kFieldMax;
    return MSSPE_OK;
}

int msspe_host_bound_window(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t info[8])
{
    // host only: the windowed instance's constants (csrc/fast_tables.hpp BoundWindow) as chem_entry() would build them
    if (!chem || !info) return MSSPE_ERR_ARG;
    for (int q = 0; q < 8; ++q) info[q] = 0;
    auto bp = std::make_unique<BoundPacked>();
    if (int rc = host_bound_packed(params_path, chem, dg_threshold, *bp)) return rc;
    BoundWindow w;
    build_bound_window(*bp, pairs_bound_window_rows(), w);
    info[0] = w.usable;
    info[1] = w.F;
    info[2] = w.ifar;
    info[3] = w.bfar;
    info[4] = BoundWindow::kVoid;
    return MSSPE_OK;
}

int msspe_host_bound_mirror_ok(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *mirror_ok)
{
    // host only: ChemEntry::mirror_ok as chem_entry() would set it
    if (!chem || !mirror_ok) return MSSPE_ERR_ARG;
    *mirror_ok = 0;
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    if (!(chem->dna_conc > 0) || chem->max_loop < 0 || chem->max_loop > 30) return MSSPE_ERR_ARG;
    const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                           chem->max_loop, false, dg_threshold);
    auto pt = std::make_unique<PairTables>();
    if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_ERR_TABLES;
    auto ft = std::make_unique<FastTables>();
    auto it = std::make_unique<IntTables>();
    auto st = std::make_unique<SplitTables>();
    const TableRoutes r = table_routes(*tb, *pt, chem->max_loop, *ft, *it, *st);
    auto bt = std::make_unique<BoundTables>();
    const bool ok = build_bound_tables(*ft, c, pairs_bound_max_k(), *bt) && r.row_ok;
    *mirror_ok = ok && bt->mirror_ok ? 1 : 0;
    return MSSPE_OK;
}

int msspe_host_split_tables(const char *params_path, const msspe_chem *chem, double *S, int32_t *H,
                            int32_t *g, int32_t *L, int32_t *X, int32_t info[4])
{
    // host only: what the long-oligo kernel keeps in LDS (csrc/split_tables.hpp)
    if (!chem || !S || !H || !g || !L || !X || !info) return MSSPE_ERR_ARG;
    auto tb = std::make_unique<NNTables>();
    std::string err;
    const std::string path = params_path && *params_path ? params_path : default_bundle_path();
    if (!load_nn_tables(path, *tb, err)) return MSSPE_ERR_TABLES;
    const ThalConsts c = make_dimer_consts(chem->mv, chem->dv, chem->dntp, chem->dna_conc, chem->temp_c,
                                           chem->max_loop, false, -9000.0f);
    auto pt = std::make_unique<PairTables>();
    if (!build_pair_tables(*tb, c, *pt, err)) return MSSPE_ERR_TABLES;
    auto st = std::make_unique<SplitTables>();
    build_split_tables(*pt, chem->max_loop, *st);
    std::memcpy(S, st->S, sizeof st->S);
    std::memcpy(H, st->H, sizeof st->H);
    std::memcpy(g, st->g, sizeof st->g);
    std::memcpy(L, st->L, sizeof st->L);
    std::memcpy(X, st->X, sizeof st->X);
    info[0] = st->usable;
    info[1] = st->max_k;
    info[2] = SplitTables::kCount;
    info[3] = SplitTables::kXCount;
    return MSSPE_OK;
}

float msspe_round_g_f32(double x) { return round_g_f32(x); }
float msspe_round_fixed_f32(double x, int decimals) { return round_fixed_f32(x, decimals); }
double msspe_g_cut(float threshold) { return g_cut(threshold); }

}  // extern "C"
