/*
 * msspe_hip.h -- C ABI of the MI355X primer-screening engine (libmsspe_hip.so).
 *
 * Drop-in boundary for od-msspe's hot path.  The reference has no library API: it reaches its
 * thermodynamic arithmetic through two child processes chosen by --ntthal / --primer3
 * (/root/reference/od-msspe/src/config.rs:142-147, :179-202).  Every entry point below replaces
 * one of those process boundaries or one in-process stage-A function, and cites it.
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add to od-msspe.
 *
 * Conventions:
 *   - every call returns an int status (MSSPE_OK = 0); msspe_last_error(ctx) gives the text;
 *   - plain pointers and sizes only, caller owns every buffer, no exceptions cross the boundary;
 *   - one context per host thread per device; calls on different contexts are concurrent-safe;
 *   - `_dev` entry points take DEVICE pointers and enqueue on the context's HIP stream; in the steady
 *     state they neither allocate nor synchronise, but the FIRST call with a new chemistry / threshold, or
 *     with a larger problem than any before, builds tables and (re)allocates work buffers, which
 *     synchronises.  Warm a context up with one call of the final size before capturing a HIP graph.  The
 *     others take HOST pointers, copy, run and synchronise;
 *   - there is NO CPU fallback: without a usable gfx950 device msspe_create() fails.
 *
 * Oligo encoding on the device: one uint64 per oligo, base p (0-based from the 5' end) in bits
 * [2p, 2p+1], A=0 C=1 G=2 T=3, k <= 32.  Oligos must be pure ACGT (stage A only emits such words,
 * od-msspe/src/main.rs:167).
 */
#ifndef MSSPE_HIP_H
#define MSSPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msspe_ctx msspe_ctx;

enum msspe_status {
    MSSPE_OK = 0,
    MSSPE_ERR_ARG = 1,      /* NULL pointer, bad range, non-ACGT oligo ...            */
    MSSPE_ERR_K = 2,        /* unsupported oligo length                               */
    MSSPE_ERR_TABLES = 3,   /* thermodynamic parameter files missing / malformed; from a
                               dimer call: an enthalpy that is not an integer or is
                               beyond 1e6 in magnitude (see msspe_create)              */
    MSSPE_ERR_DEVICE = 4,   /* HIP error (no device, launch failure, out of memory)   */
    MSSPE_ERR_CAPACITY = 5, /* caller-supplied output capacity exceeded               */
    MSSPE_ERR_NOMEM = 6
};

/* Chemistry handed to ntthal by od-msspe/src/delta_g.rs:93-110 (-mv -dv -n -d -t, all "{:.2}"
 * strings of f32) and defaults of od-msspe/src/constants.rs:7-15. */
typedef struct {
    double mv;        /* monovalent cations, mM          (--mv-conc,  50)   */
    double dv;        /* divalent cations, mM            (--dv-conc,  3)    */
    double dntp;      /* dNTP, mM                        (--dntp-conc, 0)   */
    double dna_conc;  /* oligo concentration, nM         (--dna-conc, 250)  */
    double temp_c;    /* temperature dG is reported at   (--annealing-temp, 25) */
    int max_loop;     /* ntthal -maxloop, 30                                 */
} msspe_chem;

void msspe_chem_ntthal_defaults(msspe_chem *c);   /* 50 / 3 / 0 / 250 nM / 25 C  */
void msspe_chem_primer3_defaults(msspe_chem *c);  /* 50 / 1.5 / 0.6 / 50 nM / 37 C: what
                                                     primer3_core uses for od-msspe's records
                                                     (od-msspe/src/primer.rs:125-140)        */

/* ---- context ---------------------------------------------------------------------------- */

/* device: HIP device ordinal.  params_path: a Primer3-format directory (what ntthal gets via
 * `-path`, od-msspe/src/delta_g.rs:90,107-108), or a consolidated bundle file, or NULL for the
 * bundle shipped next to the library.
 *
 * The files are read as they are and every kernel computes with what they hold; which kernel answers
 * a pair is decided from them, per chemistry (msspe_host_table_routes reads the decision):
 *   - every finite enthalpy an integer of magnitude at most 1e6: gates everything.  Otherwise every
 *     dimer call (ANY, END, _ab, edges, cover, tubes, detail, background thal / amplicons, and the
 *     self-dimers of msspe_oligo_stats*; its Tm, GC % and HAIRPIN_TH asked for without them are
 *     served) returns MSSPE_ERR_TABLES and msspe_last_error says "not
 *     integral", where ntthal would compute; msspe_create itself succeeds and the context stays
 *     usable.
 *   - fast_ok (H a multiple of 10, every Watson-Crick stack exists, the entropy clamp out of reach for
 *     16-mers, loop rows fit): the register-table f64 kernels, the END screen's first stage, one-lane
 *     self-dimers.  A missing Watson-Crick stack also sets split_max_k and wave_max_k to 0: only the
 *     dense kernel restates thal.c's rule for it.
 *   - int_ok (also S on the 0.01 grid and int32 ranges within reach): the integer first stage and
 *     the integer list stage.
 *   - row_ok (also every end term and Watson-Crick stack exists): the row kernel, and the general
 *     integer kernel's assumption that every complementary cell is reachable.  End terms always exist
 *     (the bare closing pair at the least) and a missing Watson-Crick stack clears fast_ok, so with the
 *     present builders row_ok equals int_ok.
 *   - split_max_k, 0 to 32 (int32 and 16-bit biased-H ranges, checked per length): the split-table
 *     kernel up to that length.
 *   - wave_max_k, 0 to 32 (entropy cutoff out of reach, checked per length): one wave per pair up to
 *     that length; above it the dense kernel.
 * A route that is not exact for a table stands down; the results are the same doubles on every route. */
int msspe_create(int device, const char *params_path, msspe_ctx **out);
void msspe_destroy(msspe_ctx *ctx);
const char *msspe_last_error(const msspe_ctx *ctx);
const char *msspe_version(void);
/* Use the caller's hipStream_t (e.g. PyTorch's current stream) for every later call; NULL is
 * HIP's default (null) stream.  msspe_reset_stream() returns to the context's own stream. */
/* Engine options: which kernels later calls may use.  Nothing in the library reads the process
 * environment; the defaults are the product path and the other values exist so that the parity tests
 * can run every stage against every other (the reference has no equivalent: its only knobs are the
 * --ntthal / --primer3 paths, od-msspe/src/config.rs:142-147).  Unknown key / bad value: MSSPE_ERR_ARG.
 *   "pair_kernel"    "auto" | "f64" (f64 register-table kernel first) | "int" (general integer kernel first)
 *   "force_generic"  "0" | "1"    dense one-lane-per-pair kernels only
 *   "split_min_k"    "2".."99"    shortest oligo that goes to the split-table kernel (16; 14- and 15-mers run the row-specialised first stage)
 *   "wave_kernel"    "0" | "1"    one-wave-per-pair f64 kernel in the chain (1)
 *   "list_cap_log2"  "0" | "20".."30"   fixed hand-over list size (0: sized by the call)
 *   "site_list_cap_log2" "12".."26"  msspe_background_thal* and msspe_segment_coverage_thal*: the work list holds
 *                                 2^this sites or matches (22)
 *   "amplicon_keys_cap_log2" "10".."28"  msspe_background_amplicons*: the stable-key buffer of a context is first
 *                                 made with 2^this keys (20) and doubles as needed; no result depends on it
 *   "panel_thin_matrix_max_mb" "1".."1048576"  msspe_panel_thin*: the most its incidence matrix may take, in MB
 *                                 (8192); a call that needs more returns MSSPE_ERR_CAPACITY
 *   "thin_thal_unique" "0" | "1"  msspe_panel_thin_thal*: score each distinct (primer, template) pair of a slab once
 *                                 (1) or every match (0); no result depends on it
 *   "conflict_graph_block_rows" "0" | a positive number  msspe_conflict_graph* under both rules: rows per block of
 *                                 the two per-rule planes in the context's scratch (0, auto: as many as keep both
 *                                 planes within 64 MB); no result depends on it
 *   "split_lanes"    "0" | "2" | "4" | "8"
 *   "split_list"     "0" | "1"    short oligos: tables too large for the integer list stage go to the split-table
 *                                 kernel's list mode (1) or straight to the f64 kernels (0)
 *   "short_chain"    "0" | "1"    screen blocks of up to 2^23 pairs: the integer list stage hands straight to one wave
 *                                 per pair (1), or the block takes the long chain of larger blocks (0)
 *   "row_oob"        "0" | "1"    the row-specialised first stage, which reads LDS beyond its allocation and takes the
 *                                 0 gfx950 returns there for "not available" (1; it also needs the per-engine probe to
 *                                 pass), or the general integer kernel, which never leaves its allocation (0: for
 *                                 debugger / trap-handler sessions that raise MEM_VIOL on such reads)
 *   "pair_bound"     "auto" | "0" | "1"  the BOUND first stage.  A screen that asks for decisions only (counts, bitmap:
 *                                 no dG plane, no Tm plane, no edge list) of oligos of up to 13 bases with a cut <= 0,
 *                                 where the row-specialised first stage would run, may run a cheaper instance of it
 *                                 first: a lower bound of every dG thal() could report for the pair (the minimum over
 *                                 all chains of stacked pairs and loops, at the chemistry's temperature, in integers
 *                                 rounded down).  A pair whose bound is more than 1 cal/mol above the cut cannot
 *                                 conflict and is finished; every other pair goes to hand-over list 0 and is answered
 *                                 by the exact stages, so every decision is the one the exact kernels make.
 *                                 "1": wherever it applies; "0": never; "auto" (default): while the share of pairs it
 *                                 cannot cull stays below half the break-even share -- measured once per chemistry,
 *                                 threshold and oligo length by a probe launch over at most 2^20 pairs of the first
 *                                 such call's block (one extra host round trip, none when the stream is being captured:
 *                                 the exact kernel then runs)
 *   "pair_mirror"    "auto" | "0" | "1"  where the bound first stage runs on a square same-pool block (rows = columns) and
 *                                 its tables are strand-symmetric term by term (msspe_host_bound_mirror_ok), it fills
 *                                 each unordered pair once -- the bound of (a, b) is one of (b, a) too -- and hands a
 *                                 pair it cannot cull on in both orders ("auto", the default, and "1": the same; the
 *                                 mirror is never applied where it is not proven); "0": every ordered pair is filled
 *   "pair_bound_list" "auto" | "0" | "1"  where the bound first stage runs, a lane that leaves its wave WITHOUT a bound of
 *                                 its own (53..63 stored cells, dragged, shed by the slot fit) goes to a list of its own,
 *                                 once per unordered pair under the mirror, and gets the same bound from a list kernel
 *                                 (k_pairs_bound_list) before the exact list stages; what that cannot cull joins hand-over
 *                                 list 0 ("auto", the default, and "1": the same); "0": such lanes go to list 0 as they
 *                                 are.  Decisions are the exact stages' either way.  msspe_get_info "bound_list_pairs" /
 *                                 "bound_list_survivors": entries that list held / ordered pairs handed on from it
 *                                 since the last read
 *   "pair_bound_packed" "auto" | "0" | "1"  where the bound first stage runs, its PACKED instance runs in its place
 *                                 (k_pairs_bound_packed: the same bound in a coarser unit of 1, 2 or 4 cal/mol, every term
 *                                 rounded down, the value in the slot word beside the coordinates -- half the slot
 *                                 registers, four waves per SIMD), wherever a proven range of the chemistry's cell values
 *                                 fits that field (msspe_host_bound_packed; "auto", the default, and "1": the same);
 *                                 "0": the exact-unit instance.  A coarser bound only culls fewer pairs; decisions are
 *                                 the exact stages' either way
 *   "pair_bound_window" "auto" | "0" | "1"  where the packed instance runs and "pair_bound_list" is on, its WINDOWED
 *                                 instance runs in its place (k_pairs_bound_window): a cell of row i scans the rows
 *                                 i-F .. i-1 and takes one candidate, built on the smallest value of all rows above and
 *                                 the cheapest long-loop entries (msspe_host_bound_window), for the rest -- a lower bound
 *                                 of the packed instance's value at fewer instructions.  A pair it cannot cull goes to
 *                                 the bound list stage's list, whose exact-unit bound decides before the exact stages.
 *                                 "1": wherever that applies; "auto" (the default): the same for screens of 2^23 pairs
 *                                 and more; "0": never.  msspe_get_info "bound_window_survivors": ordered pairs it sent
 *                                 to that list as not culled since the last read ("bound_survivors" counts what the
 *                                 exact-unit and packed instances append to hand-over list 0; the windowed one appends
 *                                 none, behind it "bound_list_survivors" holds the pairs no bound could cull)
 *   "pair_bound_list_packed" "auto" | "0" | "1"  where the bound list stage runs behind the packed or the windowed first
 *                                 stage, its PACKED instance runs in its place (k_pairs_bound_list_packed: the packed first
 *                                 stage's unit, tables and cull rule, the value in the slot word beside the coordinates --
 *                                 half the slot registers, four waves per SIMD).  A pair of that list then meets the very
 *                                 bound the packed first stage applies to the pairs it keeps.  "1": wherever that
 *                                 applies; "auto" (the default): the same for screens of 2^23 pairs and more; "0": the
 *                                 exact-unit list kernel.  A coarser bound only culls fewer pairs; decisions are the exact
 *                                 stages' either way
 *   "stage_a_graph" "0" | "1"   hipGraph replay of stage A's greedy loop (1)
 *   "stage_a_candidates" "0" | "1"  greedy loop over the list of words near the maximum (1), or over all the
 *                                 words on every iteration (0); the winners are the same */
int msspe_set_option(msspe_ctx *ctx, const char *key, const char *value);
/* Facts about the context's device and what it will run (engine-only diagnostics, no reference counterpart):
 *   "device"          HIP ordinal           "n_cu"  compute units
 *   "lds_reads_zero"  1: the per-engine probe found that LDS reads beyond a block's allocation return 0 (every
 *                     gfx950 seen), i.e. the row-specialised first stage may run; 0: the general kernel runs
 *   "row_kernel"      1: 13-mer pools go to the row-specialised first stage with the current options and the
 *                     tables of every chemistry this context has met (0 once a call found row_ok unset: see msspe_create)
 *   "stage_a_fast_iterations" / "stage_a_general_iterations" / "stage_a_rebuilds" / "stage_a_idle_iterations"
 *                     the last msspe_kmer_candidates* call's greedy loop: iterations that recorded winners from the
 *                     partitions' leaders alone / after a walk over posting lists, candidate lists made, idle
 *                     iterations at the end of the last batch
 *   "site_list_cap_log2"  the option's current value
 *   "background_thal_slabs" / "background_thal_redone"
 *                     the last msspe_background_thal* call: slabs scored, and slabs whose sites did not fit the work
 *                     list and were split and listed again
 *   "background_thal_flank_classes" / "background_thal_truncated"
 *                     the last scored call (msspe_background_thal* / _amplicons*, with or without a flank): distinct
 *                     (fl, fr) classes that were scored (1 at flank 0 when there were sites), and sites whose template
 *                     found fewer than `flank` base columns on either side
 *   "amplicon_keys_cap_log2"  the option's current value
 *   "amplicon_keys" / "amplicon_key_grows"
 *                     the last msspe_background_amplicons* call: stable keys it joined, and doublings of the key
 *                     buffer on the way
 *   "amplicon_sort_us" / "amplicon_join_us"
 *                     the same call's device time of the key sort with the record ids, and of the join
 *   "coverage_thal_matches" / "coverage_thal_slabs" / "coverage_thal_redone"
 *                     the last msspe_segment_coverage_thal* call: matches scored, slabs scored, and slabs whose
 *                     matches did not fit the work list and were split and listed again
 *   "coverage_thal_list_us" / "coverage_thal_score_us" / "coverage_thal_fold_us"
 *                     the same call's device time of its phases, summed over the slabs: the match listing (split
 *                     slabs included), template oligos and thal, the fold with the per-primer counts
 *   "cover_rounds"    the last msspe_conflict_cover* call: rounds that deleted nodes
 *   "cover_keys_us" / "cover_symmetrise_us" / "cover_rounds_us"
 *                     the same call's device time of its phases: sort and keys, S = B | B^T, the rounds
 *   "tube_rounds"     the last msspe_conflict_tubes* call: rounds that decided nodes
 *   "tube_keys_us" / "tube_symmetrise_us" / "tube_rounds_us"
 *                     the same call's device time of its phases: sort and keys, S = B | B^T, the keys, waits and rounds
 *   "panel_thin_matrix_max_mb"  the option's current value
 *   "panel_thin_rounds"  the last msspe_panel_thin* call: rounds that ran (its picks and the round that stopped)
 *   "panel_thin_groups"  the same call's segment groups (rows of the incidence matrix)
 *   "panel_thin_incidence_us" / "panel_thin_gain0_us" / "panel_thin_rounds_us"
 *                     the same call's device time of its phases: the incidence pass, the forced rows and first gains,
 *                     the rounds
 *   "panel_thin_depth_shadows" / "panel_thin_depth_colsum_us"
 *                     the last msspe_panel_thin_depth* / msspe_panel_thin_thal_depth* call: primers left out as
 *                     duplicates of a word, device time of the column-sum passes
 *   "hand_over_list_0" .. "hand_over_list_6"
 *                     pairs that entered hand-over list q of the cross-dimer calls (ANY and END) since the last read
 *                     of that key; reading synchronises the context's stream and resets the key, as
 *                     msspe_last_overflow_pairs does.  The first stage writes list 0; the stage that reads list q
 *                     writes list q + 1.  Which stage reads list q depends on the route:
 *                       long chain (integer first stage, up to 15 bases; blocks above 2^23 pairs, or short_chain 0),
 *                       split_list 1 and the split tables cover the length:
 *                         0 integer list stage, 1 split-table list mode, 2 f64 56-slot list stage, 3 wide table,
 *                         4 one wave per pair, 5 dense kernel (wave_kernel 0: 4 dense kernel)
 *                       long chain, split_list 0:
 *                         0 integer list stage, 1 f64 56-slot list stage, 2 wide table, 3 one wave per pair,
 *                         4 dense kernel (wave_kernel 0: 3 dense kernel)
 *                       short chain (blocks of up to 2^23 pairs, short_chain 1, wave_kernel 1):
 *                         0 integer list stage, 1 one wave per pair, 2 dense kernel
 *                       register-table first stage (pair_kernel "f64", tables without an integer image, END screen):
 *                         0 wide table, 1 one wave per pair, 2 dense kernel (wave_kernel 0: 1 dense kernel)
 *                       split-table first stage (split_min_k and up, max_loop below 2k - 4, rectangles):
 *                         0 one wave per pair, 1 dense kernel (wave_kernel 0: 0 dense kernel)
 *                       one wave per pair as the first stage (matrix mode): 0 dense kernel
 *                       force_generic: no list */
int msspe_get_info(msspe_ctx *ctx, const char *key, long long *value_out);
int msspe_set_stream(msspe_ctx *ctx, void *hip_stream);
int msspe_reset_stream(msspe_ctx *ctx);
int msspe_synchronize(msspe_ctx *ctx);

/* ---- packing ------------------------------------------------------------------------------ */

/* ASCII (n oligos x k chars, no separators) -> packed uint64.  Host-side helper. */
int msspe_pack_oligos(const char *ascii, int n, int k, uint64_t *packed_out);
void msspe_unpack_oligo(uint64_t packed, int k, char *ascii_out /* k+1 bytes */);

/* ---- stage C: all-pairs cross-dimer (replaces run_ntthal, od-msspe/src/delta_g.rs:83-153) - */

/*
 * Evaluates thal ANY (Primer3 2.6.1, what `ntthal -a ANY` computes per input line) for every
 * ORDERED pair (a = pool[i], b = pool[j]), i in [row0,row1), j in [col0,col1), self pairs
 * included (od-msspe/src/delta_g.rs:64-78), and applies the reference's decision
 * "%g-rounded dG parsed as f32 < threshold" (od-msspe/src/delta_g.rs:33-36).
 *
 * Outputs (each optional, device pointers):
 *   row_conflicts  uint32[n]            += number of conflicting columns for each row i
 *   bitmap         uint64[(row1-row0) * words], words = ceil((col1-col0)/64): bit (j-col0) of
 *                  row (i-row0) set iff (i,j) conflicts; the block is cleared by the call and
 *                  conflicts (rare) are then set with atomic ORs
 *   dg             double[(row1-row0)*(col1-col0)] raw dG in cal/mol before %g rounding;
 *                  +inf where thal finds no structure (ntthal prints nothing for such a pair;
 *                  this engine defines "no edge")
 *   tm             double[...] melting temperature t (Celsius), 0 where no structure
 * A call without the dg / tm planes asks for decisions only: where thal()'s terminal pick is a tie that doubles
 * would settle by rounding, such a call may let the pair stand as "no conflict" without settling it, if no
 * structure of the tie can reach the cut.  The bits, counts and edges are the same either way.
 */
int msspe_cross_dimer_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k,
                          const msspe_chem *chem, float dg_threshold,
                          int row0, int row1, int col0, int col1,
                          uint32_t *d_row_conflicts, uint64_t *d_bitmap, double *d_dg,
                          double *d_tm);

/* Host-buffer convenience: packs, uploads, runs the full n x n matrix, downloads. */
int msspe_cross_dimer(msspe_ctx *ctx, const char *pool_ascii, int n, int k,
                      const msspe_chem *chem, float dg_threshold,
                      uint32_t *row_conflicts, uint64_t *bitmap, double *dg, double *tm);

/* The same screen as an edge list (the reference keeps one edge with its dG per conflicting
 * ordered pair, od-msspe/src/delta_g.rs:33-46, and reads it back through Edge::get_dg(), :10-15).
 *   _dev: enqueue only.  d_edges[capacity] receives (a, b, raw double dG) in no particular order, *d_count the
 *         number of conflict edges of the block; a count above the capacity means the list is truncated (the
 *         first `capacity` to arrive are kept).  d_row_conflicts optional.
 *   host: whole pool; edges sorted by (a, b) as the reference's nested loops produce them, dg = the value
 *         get_dg() yields ("%g" -> f32 -> "{:.2}" -> f32).  *count_out = number of conflict edges; when it
 *         exceeds `capacity` the call returns MSSPE_ERR_CAPACITY with the first `capacity` edges (of the
 *         arrival order, then sorted) filled in, so the caller can retry with count_out entries. */
typedef struct {
    uint32_t a, b;   /* pool indices of the ordered pair */
    double dg;       /* cal/mol, unrounded */
} msspe_edge_dev;
typedef struct {
    uint32_t a, b;
    float dg;
} msspe_edge;
int msspe_cross_dimer_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                float dg_threshold, int row0, int row1, int col0, int col1,
                                uint32_t *d_row_conflicts, msspe_edge_dev *d_edges, uint64_t capacity,
                                uint64_t *d_count);
int msspe_cross_dimer_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                            float dg_threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out);
/* Diagnostic (tests and debugging; no screen reads it): what the bound first stage (option "pair_bound") computes
 * for every ordered pair of the block, as a double in cal/mol in the caller's plane d_bound[(row1-row0) * (col1-col0)]
 * (layout of msspe_cross_dimer_dev's dG plane): a value <= every dG thal() can report for the pair + 1 cal/mol; +inf
 * where the pair has no complementary base pair at all; -inf for a pair that stage does not bound but hands on as it is
 * (more stored cells than its table holds, both oligos self-complementary).  Asynchronous on the context's stream.
 * MSSPE_ERR_ARG where the stage does not apply: k > 13, a threshold whose cut is above 0, tables it cannot hold. */
int msspe_cross_dimer_bound_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound);
/* The same plane from the PACKED instance of the bound first stage (option "pair_bound_packed"): the same pairs carry
 * a value, +inf and -inf; a value is an integer multiple of the instance's unit (1, 2 or 4 cal/mol) and at most the
 * exact-unit instance's.  MSSPE_ERR_ARG also where the chemistry's range of cell values fits none of those units. */
int msspe_cross_dimer_bound_packed_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                       float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound);
/* The same plane from the WINDOWED packed instance (option "pair_bound_window"): the same pairs carry a value, +inf and
 * -inf; a value is a multiple of the packed instance's unit and at most the packed instance's.  MSSPE_ERR_ARG also where
 * msspe_host_bound_window reports usable = 0. */
int msspe_cross_dimer_bound_window_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                       float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound);
/* The same plane with the bound LIST stage (option "pair_bound_list") behind the first stage: every pair the first stage
 * would put on list U -- 53..63 stored cells, lanes dragged or shed from their wave -- carries the value that stage
 * computes for it (the same recurrence on the same integer terms) instead of -inf.  -inf remains exactly for pairs of two
 * self-complementary oligos and pairs with more than 63 stored cells, +inf for pairs without a complementary base pair.
 * The block may hold at most as many pairs as a hand-over list (2^20 .. 2^30: it grows with the call). */
int msspe_cross_dimer_bound_list_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                     float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound);
/* The same plane from the PACKED instances of both stages (options "pair_bound_packed" and "pair_bound_list_packed"):
 * the same pairs carry a value, +inf and -inf as in msspe_cross_dimer_bound_list_dev; every value is an integer multiple of
 * the packed unit (1, 2 or 4 cal/mol).  MSSPE_ERR_ARG also where the chemistry's range of cell values fits none of those
 * units. */
int msspe_cross_dimer_bound_list_packed_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                            float dg_threshold, int row0, int row1, int col0, int col1, double *d_bound);

/* One pool screened against another (engine extension: the reference screens one pool of one --kmer-size,
 * od-msspe/src/delta_g.rs:61-81; ntthal itself takes any two oligos).  Pool A: n_a oligos of k_a bases, oligo 1
 * (the rows); pool B: n_b oligos of k_b bases, oligo 2 (the columns); k_a, k_b in 2..32 and free to differ.  Only
 * the ordered pairs (A[i], B[j]), i in [row0,row1) of A, j in [col0,col1) of B, are evaluated: for (B[j], A[i])
 * swap the pools.  Outputs, decision, +inf / 0 for no structure and the clearing of the bitmap block are those of
 * msspe_cross_dimer_dev, with rows indexing A and columns indexing B (row_conflicts: uint32[n_a] +=).
 * k_a == k_b runs the single-pool chain on A and B staged back to back in a context-owned buffer (same results by
 * construction); k_a != k_b runs the rectangular chain.  Empty pools or blocks: MSSPE_OK. */
int msspe_cross_dimer_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                             int k_b, const msspe_chem *chem, float dg_threshold, int row0, int row1, int col0,
                             int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap, double *d_dg, double *d_tm);
/* The same block as an edge list, contract of msspe_cross_dimer_edges_dev; an edge's a is an A index, b a B index. */
int msspe_cross_dimer_ab_edges_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b,
                                   int n_b, int k_b, const msspe_chem *chem, float dg_threshold, int row0, int row1,
                                   int col0, int col1, uint32_t *d_row_conflicts, msspe_edge_dev *d_edges,
                                   uint64_t capacity, uint64_t *d_count);
/* Host-buffer convenience: whole pools (a_ascii: n_a x k_a chars, b_ascii: n_b x k_b chars, no separators);
 * row_conflicts[n_a], bitmap[n_a * ceil(n_b/64)], dg / tm [n_a * n_b], each optional.  Non-ACGT: MSSPE_ERR_ARG. */
int msspe_cross_dimer_ab(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b, int k_b,
                         const msspe_chem *chem, float dg_threshold, uint32_t *row_conflicts, uint64_t *bitmap,
                         double *dg, double *tm);
/* The same pools as an edge list: a = A index, b = B index, sorted by (a, b), Edge::get_dg() rounding and the
 * MSSPE_ERR_CAPACITY contract of msspe_cross_dimer_edges. */
int msspe_cross_dimer_ab_edges(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                               int k_b, const msspe_chem *chem, float dg_threshold, msspe_edge *edges, uint64_t capacity,
                               uint64_t *count_out);
/* One pool whose oligos may differ in length (NUL-terminated, 2..32 bases each): every ordered pair, self pairs
 * included, edges sorted by (a, b) with Edge::get_dg() rounding -- msspe_cross_dimer_edges for what ntthal
 * accepts; same MSSPE_ERR_CAPACITY contract.  The oligos are grouped by length and every (row length, column
 * length) block is screened as above; a pool of one length gives exactly msspe_cross_dimer_edges's list. */
int msspe_cross_dimer_edges_mixed(msspe_ctx *ctx, const char *const *oligos, int n, const msspe_chem *chem,
                                  float dg_threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out);

/* ---- stage C, 3'-end dimers: thal END1 for every ordered pair (ntthal -a END1 / -a END2) ------ */

/*
 * The END screen: Primer3 2.6.1 thal type END1 (structures that close on the 3' base of oligo 1 = the row; without
 * one, thal's fallback to cell (1, 1)) for every ORDERED pair of the block, self pairs included -- the pair
 * analogue of the SELF_END_TH filter od-msspe applies to each primer (od-msspe/src/main.rs:498-499).  END2(a, b) is
 * END1(b, a): one screen answers both 3' ends, and max(T, T^T) of its t plane T is the per-pair maximum.
 * Decision: a pair conflicts iff !(round_fixed_f32(t_end, 2) < tm_threshold), t_end = max(0, t), 0 without a
 * structure (od-msspe's SELF_END rule); tm_threshold <= 0: every pair conflicts.  The kernels test
 * t_end > msspe_t_cut(tm_threshold).
 * Outputs as msspe_cross_dimer_dev: row_conflicts +=, bitmap block cleared by the call, dg = raw dG (+inf without a
 * structure), tm = raw t (0 without a structure).  A call without planes gives the same bits (the f64 kernels settle
 * terminal-pick ties in Primer3's order).
 * Kernels: the f64 register-table kernel (equal lengths, k <= 16, max_loop >= 2k - 4), else the one-wave-per-pair
 * kernel, then the dense kernel.  Options force_generic, wave_kernel and list_cap_log2 apply;
 * pair_kernel, split_min_k, split_lanes and row_oob do not (there is no integer END stage).
 * Argument errors return the statuses of the thal ANY sibling.
 */
int msspe_cross_dimer_end_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                              float tm_threshold, int row0, int row1, int col0, int col1, uint32_t *d_row_conflicts,
                              uint64_t *d_bitmap, double *d_dg, double *d_tm);
/* Host-buffer convenience: packs, uploads, runs the full n x n matrix, downloads (as msspe_cross_dimer). */
int msspe_cross_dimer_end(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                          float tm_threshold, uint32_t *row_conflicts, uint64_t *bitmap, double *dg, double *tm);
/* The END screen as an edge list.
 *   _dev: contract of msspe_cross_dimer_edges_dev; a record carries the raw double t of the pair.
 *   host: whole pool, edges sorted by (a, b), t = round_fixed_f32(t_end, 2) (the "%.2f" value the decision reads),
 *         MSSPE_ERR_CAPACITY contract of msspe_cross_dimer_edges. */
typedef struct {
    uint32_t a, b;   /* pool indices of the ordered pair (a = oligo 1, the anchored 3' end) */
    double t;        /* Celsius, unrounded (0 without a structure) */
} msspe_end_edge_dev;
typedef struct {
    uint32_t a, b;
    float t;
} msspe_end_edge;
int msspe_cross_dimer_end_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                    float tm_threshold, int row0, int row1, int col0, int col1,
                                    uint32_t *d_row_conflicts, msspe_end_edge_dev *d_edges, uint64_t capacity,
                                    uint64_t *d_count);
int msspe_cross_dimer_end_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                                float tm_threshold, msspe_end_edge *edges, uint64_t capacity, uint64_t *count_out);
/* Pool A (oligo 1, the anchored 3' end) against pool B (oligo 2), lengths 2..32 and free to differ: the END screen
 * over the pairs (A[i], B[j]) with the staging, block and output conventions of msspe_cross_dimer_ab_dev /
 * msspe_cross_dimer_ab.  END2 of (A[i], B[j]): swap the pools. */
int msspe_cross_dimer_end_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                                 int k_b, const msspe_chem *chem, float tm_threshold, int row0, int row1, int col0,
                                 int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap, double *d_dg, double *d_tm);
int msspe_cross_dimer_end_ab(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                             int k_b, const msspe_chem *chem, float tm_threshold, uint32_t *row_conflicts,
                             uint64_t *bitmap, double *dg, double *tm);

/* ---- the conflict graph under a pair of rules: thal ANY on dG and / or thal END1 on t ---- */

/*
 * A pair conflicts when at least one enabled rule says so.  Each rule's decision is exactly that of its screen on the
 * same block under the same chemistry and threshold: use_any -- msspe_cross_dimer*'s with dg_threshold; use_end --
 * msspe_cross_dimer_end*'s with end_tm_threshold, the row being oligo 1 (the anchored 3' end).
 */
typedef struct {
    int   use_any;  float dg_threshold;       /* thal ANY, msspe_cross_dimer*'s decision            */
    int   use_end;  float end_tm_threshold;   /* thal END1, msspe_cross_dimer_end*'s decision; row = oligo 1 */
} msspe_conflict_rule;
#define MSSPE_KIND_ANY 1u
#define MSSPE_KIND_END 2u
typedef struct { uint32_t a, b, kinds, reserved; } msspe_kind_edge;   /* reserved = 0 */

/*
 * The block [row0,row1) x [col0,col1) of one pool under the rule.  Outputs (device pointers, each may be NULL):
 *   d_row_conflicts  uint32[n]   [r] += the set bits of row r in the block; a pair under both rules counts once
 *   d_bitmap         uint64[(row1-row0) * ceil((col1-col0)/64)], the block layout of msspe_cross_dimer_dev: cleared by
 *                    the call, then written; words outside the block are not touched.  As in msspe_cross_dimer_dev the
 *                    block's words are cleared whole, so the padding bits of a row's last word end as 0.
 *   d_kind_counts    uint64[3]   += the block's pairs that are ANY only, END only, and both
 * use_any && !use_end: bit for bit the bitmap and counts of a decisions-only msspe_cross_dimer_dev -- with a bitmap or
 * without kind counts the call IS that screen on the caller's buffers (same route, every option applies);
 * !use_any && use_end: those of msspe_cross_dimer_end_dev, likewise.  With both rules the two per-rule bitmaps live in
 * context-owned scratch, a block of rows at a time: msspe_set_option "conflict_graph_block_rows" (0 = auto: as many
 * rows as keep both planes within 64 MB; any positive value is honoured).  Results do not depend on it, and once the
 * scratch has grown to a call's size no further allocation happens (msspe_get_info "conflict_graph_grows" counts
 * them).  Enqueues on the context's stream; synchronises no more than the two screens do.
 * Errors: a NULL rule, a NULL chem or both flags zero: MSSPE_ERR_ARG; every other argument status is that of
 * msspe_cross_dimer_dev.  n == 0 or an empty block: MSSPE_OK, nothing written.
 */
int msspe_conflict_graph_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                             const msspe_conflict_rule *rule, int row0, int row1, int col0, int col1,
                             uint32_t *d_row_conflicts, uint64_t *d_bitmap, uint64_t *d_kind_counts);
/* Pool A (rows; oligo 1 of the END rule) against pool B (columns), lengths 2..32 and free to differ: the staging and
 * block conventions of msspe_cross_dimer_ab_dev. */
int msspe_conflict_graph_ab_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b, int n_b,
                                int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule, int row0, int row1,
                                int col0, int col1, uint32_t *d_row_conflicts, uint64_t *d_bitmap,
                                uint64_t *d_kind_counts);
/* The block as an edge list: every set bit as (a, b, kinds) in ascending (a, b) order -- the kernel produces the order
 * itself, nothing is sorted afterwards.  *d_count = the number of edges of the block, cleared by the call; it may
 * exceed `capacity`, in which case d_edges holds the first `capacity` edges of the order and nothing is written
 * behind them.  Edges carry no dG or t: the single-rule edge screens give values.  d_row_conflicts, d_bitmap and
 * d_kind_counts optional, as above.  A NULL d_count, or a capacity without a buffer: MSSPE_ERR_ARG. */
int msspe_conflict_graph_edges_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const msspe_chem *chem,
                                   const msspe_conflict_rule *rule, int row0, int row1, int col0, int col1,
                                   uint32_t *d_row_conflicts, uint64_t *d_bitmap, uint64_t *d_kind_counts,
                                   msspe_kind_edge *d_edges, uint64_t capacity, uint64_t *d_count);
int msspe_conflict_graph_ab_edges_dev(msspe_ctx *ctx, const uint64_t *d_a, int n_a, int k_a, const uint64_t *d_b,
                                      int n_b, int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule,
                                      int row0, int row1, int col0, int col1, uint32_t *d_row_conflicts,
                                      uint64_t *d_bitmap, uint64_t *d_kind_counts, msspe_kind_edge *d_edges,
                                      uint64_t capacity, uint64_t *d_count);
/* Host pool, whole n x n: row_conflicts[n], bitmap[n * ceil(n/64)] and kind_counts[3] are host buffers, each optional,
 * and are assigned (not added to).  Non-ACGT: MSSPE_ERR_ARG. */
int msspe_conflict_graph(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                         const msspe_conflict_rule *rule, uint32_t *row_conflicts, uint64_t *bitmap,
                         uint64_t *kind_counts);
/* Host edge lists, whole pool(s), ascending (a, b).  *count_out = the number of edges; above `capacity` the call
 * returns MSSPE_ERR_CAPACITY with the first `capacity` edges filled in, so the caller can retry with count_out. */
int msspe_conflict_graph_edges(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                               const msspe_conflict_rule *rule, msspe_kind_edge *edges, uint64_t capacity,
                               uint64_t *count_out);
int msspe_conflict_graph_ab_edges(msspe_ctx *ctx, const char *a_ascii, int n_a, int k_a, const char *b_ascii, int n_b,
                                  int k_b, const msspe_chem *chem, const msspe_conflict_rule *rule,
                                  msspe_kind_edge *edges, uint64_t capacity, uint64_t *count_out);

/* ---- the greedy vertex cover of the conflict graph (replaces vertex_cover, od-msspe/src/main.rs:754-798) ---- */

/*
 * The primers the reference's cover removes: nodes are the oligos of the pool (distinct), v and u are neighbours when
 * (v, u) or (u, v) conflicts (the graph is symmetrised: thal ANY is not symmetric), and a self conflict puts v among
 * its own neighbours.  Repeatedly the node with the most live neighbours is deleted, ties going to the
 * lexicographically greatest oligo, until no live node has a live neighbour.  The device computes the same set in
 * rounds that delete every local maximum of the key (live degree, lexicographic rank) at once.
 * drop_self_pairs: the reference's --check-self-dimers false -- the pairs (a, a) and (a, revcomp(a)) are never edges
 * (od-msspe/src/delta_g.rs:64-69).
 * Errors: the argument statuses of msspe_cross_dimer* (NULL pointers, k outside 2..32: MSSPE_ERR_K, non-ACGT), and
 * MSSPE_ERR_ARG for duplicate oligos, a pool word with bits above 2 k, or n above 262,144 (the symmetrised bitmap the
 * cover keeps in the context is n^2 / 8 bytes).  An allocation failure is MSSPE_ERR_DEVICE.  n == 0: MSSPE_OK, nothing
 * deleted.  msspe_get_info "cover_rounds" gives the number of rounds of the last call.
 *
 * d_bitmap: n x ceil(n/64) words, the layout msspe_cross_dimer_dev writes for the full block [0,n) x [0,n) (read
 * only).  d_deleted[n] (device bytes): 1 = removed by the cover.  Enqueues; synchronises once per batch of rounds.
 * n_deleted_out (host, optional): number of deleted nodes. */
int msspe_conflict_cover_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k,
                             const uint64_t *d_bitmap, int drop_self_pairs,
                             uint8_t *d_deleted, int *n_deleted_out);
/* Host pool: screens the whole pool on the device (msspe_cross_dimer_dev, bitmap only, decisions path) and covers it
 * there; no edge list is built.  deleted_out[n] host bytes. */
int msspe_conflict_cover(msspe_ctx *ctx, const char *pool_ascii, int n, int k,
                         const msspe_chem *chem, float dg_threshold, int drop_self_pairs,
                         uint8_t *deleted_out, int *n_deleted_out);
/* msspe_conflict_cover with the rule in place of dg_threshold: the pool is screened with msspe_conflict_graph_dev
 * (bitmap only) and the bitmap handed to msspe_conflict_cover_dev.  That form symmetrises to S = B | B^T, so with the END
 * rule two primers are neighbours when either order conflicts under ANY or either 3' end is caught (END1 or END2).
 * drop_self_pairs clears the same pairs: (a, a) and (a, revcomp a).  A NULL rule or both flags zero: MSSPE_ERR_ARG. */
int msspe_conflict_cover_rule(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                              const msspe_conflict_rule *rule, int drop_self_pairs, uint8_t *deleted_out,
                              int *n_deleted_out);

/* ---- the conflict graph split into reaction tubes (engine extension, no reference counterpart) ---- */

#define MSSPE_TUBE_NONE 255

/*
 * Instead of deleting primers until no two survivors conflict, assign them to at most max_tubes (1..64) tubes so that
 * no two primers of one tube conflict.  The graph is msspe_conflict_cover's: the pool's distinct oligos, S = B | B^T,
 * with drop_self_pairs the diagonal and the reverse-complement partners cleared first.  A node that still conflicts
 * with itself goes to no tube (MSSPE_TUBE_NONE), constrains nobody, and nobody waits for it.  The others are visited by
 * descending key = (degree, lexicographic rank) -- the degree is the number of neighbours other than the node itself
 * and is never updated; ties go to the lexicographically greatest oligo, as in the cover -- and each takes the lowest
 * tube that holds no neighbour placed before it, or stays unplaced (MSSPE_TUBE_NONE) when every tube holds one; an
 * unplaced node constrains nobody.  The tubes in use are 0 .. used - 1, without gaps.  The device computes the same
 * assignment in rounds.  Largest degree first keeps the most primers once there are more than a few
 * tubes; it is not a better cover: at max_tubes 1 it keeps fewer primers than msspe_conflict_cover does.
 * Errors and limits: those of msspe_conflict_cover* (duplicate oligos, bits above 2 k and n above 262,144 are
 * MSSPE_ERR_ARG), and MSSPE_ERR_ARG for max_tubes outside 1..64.  n == 0: MSSPE_OK, nothing written.
 * msspe_get_info "tube_rounds" gives the number of rounds of the last call.
 *
 * d_bitmap as for msspe_conflict_cover_dev (read only).  d_tube[n] (device bytes): the tube, or MSSPE_TUBE_NONE.
 * Enqueues on the context's stream; synchronises once for the key check and once per batch of rounds.
 * n_tubes_used_out, n_unplaced_out (host, optional): tubes in use, and nodes in no tube (self-conflicting ones
 * included). */
int msspe_conflict_tubes_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap,
                             int drop_self_pairs, int max_tubes, uint8_t *d_tube,
                             int *n_tubes_used_out, int *n_unplaced_out);
/* Host pool: screens the whole pool on the device (msspe_cross_dimer_dev, bitmap only, decisions path) and assigns the
 * tubes there; no edge list is built.  tube_out[n] host bytes. */
int msspe_conflict_tubes(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                         float dg_threshold, int drop_self_pairs, int max_tubes, uint8_t *tube_out,
                         int *n_tubes_used_out, int *n_unplaced_out);
/* msspe_conflict_tubes with the rule in place of dg_threshold (as msspe_conflict_cover_rule). */
int msspe_conflict_tubes_rule(msspe_ctx *ctx, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                              const msspe_conflict_rule *rule, int drop_self_pairs, int max_tubes, uint8_t *tube_out,
                              int *n_tubes_used_out, int *n_unplaced_out);

/* Number of pairs the last cross-dimer call routed to the generic (slow) kernel because their
 * DP did not fit the fast kernel's register-resident table. */
int msspe_last_overflow_pairs(msspe_ctx *ctx, uint64_t *count_out);

/* Diagnostics of the exact-integer stages of the cross-dimer path since the last call (engine-only,
 * no reference counterpart).  out[0..7]: the matrix-mode kernel -- out[0] = pairs it did not
 * answer because Primer3's double comparisons could go either way (they are retried in list
 * mode), out[1..7] = how many of them met each reason (Tm near-tie, loop == stack/start value with
 * another enthalpy, tie between loops, rejected minimum, tie in the terminal pick, replay
 * mismatch, equal-valued alternative on the optimal path; the row-specialised matrix kernel counts every
 * winning loop candidate of positive enthalpy as a rejected minimum and leaves the entropy half of thal.c's
 * rule to the list mode).  out[8..15]: the same for the list-mode
 * kernel; out[8] is the number of pairs that needed the f64 kernels.  Reading resets the counters. */
int msspe_pair_stage_stats(msspe_ctx *ctx, uint64_t out[16]);
/* Up to 1024 of those pairs (call before msspe_pair_stage_stats, which resets the sample count):
 * out[i] = row << 40 | col << 16 | reason bits (1 Tm, 2 loop == value, 4 loop tie, 8 rejected
 * minimum, 16 pick tie, 32 replay, 64 alternative on the path). */
int msspe_pair_stage_samples(msspe_ctx *ctx, uint64_t *out, int capacity, int *n_out);
/* Host only, no device: the folded tables the all-pairs kernels keep in LDS (csrc/fast_tables.hpp),
 * so that CPU tests can restate the integer recurrence.  fast_S / fast_H / int_g: 2604 entries,
 * int_T: 239 * 64; consts = init_S, RC, salt, temp_k, g_cut, f64 tables usable, int tables usable,
 * entry count. */
int msspe_host_pair_tables(const char *params_path, const msspe_chem *chem, float dg_threshold,
                           double *fast_S, int32_t *fast_H, int32_t *int_g, int32_t *int_T,
                           double consts[8]);
/* Host only: which routes these tables open at this chemistry (see msspe_create).  out = pair tables
 * ok, fast_ok, int_ok, row_ok, split kernel usable, split_max_k, wave_max_k, 0.  Tables with a
 * non-integral enthalpy give MSSPE_OK with out[0] = 0 (every dimer call would be refused);
 * MSSPE_ERR_TABLES only when the files cannot be loaded. */
int msspe_host_table_routes(const char *params_path, const msspe_chem *chem, int32_t out[8]);
/* Host only: the first-stage launches a pair screen of rows [row0, row1) x ncols columns from pool column col0 is cut
 * into under hand-over lists of list_cap entries (csrc/screen_plan.hpp; the screens execute this very plan).
 * first_stage: 0 dense, 1 wave, 2 split, 3 f64 register table, 4 integer, 5 row, 6 bound, 7 mirrored bound (a square
 * block, row0 == col0, of at most min(2^29, list_cap / 2) oligos).  out[i] = row0, row1, col0, col1 of launch i (the
 * wave and dense kernels' columns are the pool's, the others' positions in the sorted order; the mirrored rows too),
 * the pairs it processes, the most entries it can append to hand-over list 0, 1 if the lists are flushed before it.
 * *n_out = launches; more than capacity: MSSPE_ERR_CAPACITY, nothing written. */
int msspe_host_screen_plan(int first_stage, int row0, int row1, int col0, int ncols, int64_t list_cap, int64_t *out,
                           int capacity, int *n_out);
/* Host only: how the thal-scored site passes (msspe_background_thal*, msspe_segment_coverage_thal*,
 * msspe_panel_thin_thal* and what runs through them) cut a slab -- outer range [o0, o1) (runs, or segment groups)
 * against primers [p0, p1) -- whose `count` matches overran a work list of `cap` (count > cap; csrc/slab_split.hpp, the
 * passes execute this very rule).  out[i] = o0, o1, p0, p1 of part i, in the order the parts are pushed (the last is
 * listed first).  *n_out = parts; 0: one outer element against one primer cannot be split.  More than capacity:
 * MSSPE_ERR_CAPACITY, nothing written.  An outer range of more than 2^31 - 1 elements: MSSPE_ERR_ARG. */
int msspe_host_slab_split(int64_t o0, int64_t o1, int p0, int p1, uint64_t count, uint64_t cap, int64_t *out,
                          int capacity, int *n_out);
/* Host only: the bound first stage's tables (option "pair_bound"; csrc/fast_tables.hpp BoundTables) in the layout
 * of msspe_host_pair_tables' int_g (2604 entries) and int_T (239 * 64): every term's H - temp_k * S, a stacked pair
 * and a loop with - temp_k * salt on top, in units of 1 / info[3] cal/mol rounded down; entries >= info[6] are "not
 * available".  info = usable, initiation term, cut (a pair is culled iff initiation + the minimum over its chains
 * is above it), units per cal/mol, margin in units, bound of every reachable |sum|, the void marker, longest oligo. */
int msspe_host_bound_tables(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *bound_g,
                            int32_t *bound_T, int32_t info[8]);
/* Host only: the packed bound instance's tables (option "pair_bound_packed"; csrc/fast_tables.hpp BoundPacked), same
 * layout: every finite entry of msspe_host_bound_tables' arrays floored to a unit of 2^(shift - 6) cal/mol (entry >>
 * shift), void entries as they are.  info = usable, shift (6, 7 or 8), bias (slot field = cell value + bias), lo, hi
 * (the proven range of every value a cell can publish, coarse units: 0 <= lo + bias, hi + bias <= info[7]), initiation
 * term, cut (a pair is culled iff initiation + minimum > cut; floor(exact cut / 2^shift)), largest field value.
 * usable = 0 (all else 0): the bound stage does not apply, or no shift holds the range -- the exact-unit instance runs. */
int msspe_host_bound_packed(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *packed_g,
                            int32_t *packed_T, int32_t info[8]);
/* Host only: the windowed packed instance's constants (option "pair_bound_window"; csrc/fast_tables.hpp BoundWindow).
 * info = usable, F (rows a cell scans exactly), ifar, bfar (the smallest finite entry of msspe_host_bound_packed's T over
 * the rows l1 >= F with l2 >= 1 / with l2 = 0, coarse units; info[4] where there is none), the void value.  usable = 0
 * wherever the packed instance's is, or where hi + bias reaches the largest field value. */
int msspe_host_bound_window(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t info[8]);
/* Host only: *mirror_ok = 1 when the bound first stage may fill each unordered pair of a square same-pool screen once
 * (option "pair_mirror"): its tables are usable and every real-valued term of them equals its strand-swapped partner
 * within 1e-6 cal/mol (csrc/fast_tables.hpp bound_mirror_ok). */
int msspe_host_bound_mirror_ok(const char *params_path, const msspe_chem *chem, float dg_threshold, int32_t *mirror_ok);
/* The same for the long-oligo kernel (csrc/split_tables.hpp): S / H / g hold info[2] entries, L 1024,
 * X info[3]; info = usable, longest oligo covered, entry count, X count. */
int msspe_host_split_tables(const char *params_path, const msspe_chem *chem, double *S, int32_t *H,
                            int32_t *g, int32_t *L, int32_t *X, int32_t info[4]);

/* Full thal record for explicit pairs (a_i, b_i), i < n -- what `ntthal` prints per input line
 * (od-msspe/src/delta_g.rs:206-230): dS (salt-corrected), dH, dG, t and the base pairs of the
 * traced structure.  mode 1 = ANY, 2 = END1.  Used by the ntthal protocol shim. */
typedef struct {
    double dS, dH, dG, t;
    int32_t no_structure, n_pairs;
    uint8_t ps1[32];   /* ps1[i-1] = partner position in the REVERSED oligo 2 (1-based), 0 = unpaired */
    uint8_t ps2[32];
} msspe_thal_detail;
int msspe_thal_detail_pairs(msspe_ctx *ctx, const char *a_ascii, const char *b_ascii, int n, int k,
                            const msspe_chem *chem, int mode, msspe_thal_detail *out);

/* Measurement aid: when enabled, every launch of the dominant kernel (the all-pairs kernel) is
 * bracketed by HIP events on the context's stream; msspe_profile_read() synchronises and returns
 * the number of launches and their summed device time since the last read. */
int msspe_profile_enable(msspe_ctx *ctx, int on);
int msspe_profile_read(msspe_ctx *ctx, uint64_t *launches, double *total_ms);

/* ---- stage B: per-oligo statistics (replaces check_primers -> primer3_core,
 *      od-msspe/src/primer.rs:143-166) ---------------------------------------------------- */

/*
 * For each oligo: Tm (oligotm, SantaLucia), GC %, and max(0, t) of thal ANY / END1 of the oligo
 * against itself and of thal HAIRPIN -- PRIMER_LEFT_0_{TM,GC_PERCENT,SELF_ANY_TH,SELF_END_TH,
 * HAIRPIN_TH} (od-msspe/src/primer.rs:79-111).  Raw doubles; the text rounding primer3_core /
 * od-msspe apply (%.3f / %.2f -> f32) is msspe_round_fixed_f32().
 * A negative chem->mv or dv, or a negative dntp with dv != 0, is MSSPE_ERR_ARG (oligotm's
 * OLIGOTM_ERROR; with dv == 0 oligotm zeroes dntp before it checks it).
 */
int msspe_oligo_stats_dev(msspe_ctx *ctx, const uint64_t *d_pool, int n, int k,
                          const msspe_chem *chem, double *d_tm, double *d_gc,
                          double *d_self_any, double *d_self_end, double *d_hairpin);
int msspe_oligo_stats(msspe_ctx *ctx, const char *pool_ascii, int n, int k,
                      const msspe_chem *chem, double *tm, double *gc, double *self_any,
                      double *self_end, double *hairpin);

/* ---- stage A: k-mer candidates (replaces get_segment_manager + find_candidates_kmers,
 *      od-msspe/src/main.rs:196-235, :331-406) -------------------------------------------- */

typedef struct {
    int segment_size;          /* --window-size           500 */
    int overlap_size;          /* --overlap-size          250 */
    int search_window_size;    /* --search-windows-size    50 */
    int kmer_size;             /* --kmer-size              13 */
    int max_iterations;        /* --max-iterations       1000 */
    int max_mismatch_segments; /* --max-mismatch-segments (auto rule is the caller's) */
} msspe_kmer_opt;

/*
 * seqs: n_seq aligned sequences of equal length seq_len, row-major bytes, already upper-cased
 * with U->T (od-msspe/src/main.rs:115-118).  direction 0 = head windows as-is, 1 = tail windows
 * reverse-complemented.  Winners are written in selection order: words as packed uint64 and
 * their frequency.  *n_out = number of winners (<= capacity, else MSSPE_ERR_CAPACITY).
 * words_out / freq_out / n_out are HOST buffers in both variants (at most max_iterations small
 * records); only the sequences differ (host pointer vs. device pointer).
 */
int msspe_kmer_candidates(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                          const msspe_kmer_opt *opt, int direction,
                          uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);
int msspe_kmer_candidates_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, int direction,
                              uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);

/* ---- coverage of the final primer set: replaces the per-segment string search of
 * coverage_report() (od-msspe/src/main.rs:518-594).  seqs as for msspe_kmer_candidates; fwd_words /
 * rev_words: packed primers (msspe_pack_oligos) of the two directions, any order;
 * hit_out[seq * P + partition] (host, n_seq * P bytes, P = (seq_len - segment_size) / overlap_size
 * + 1) = 1 when the segment's head window holds a forward primer or its tail window holds the
 * reverse complement of a reverse primer.  Totals per sequence / partition stay on the host. */
int msspe_segment_coverage(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                           const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                           const uint64_t *rev_words, int n_rev, uint8_t *hit_out);
int msspe_segment_coverage_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                               const uint64_t *rev_words, int n_rev, uint8_t *hit_out);

/* Staging for hosts without a HIP binding (the reference is Rust): copy a host buffer to the
 * context's device once and use the *_dev entry points on it (the alignment is read by both
 * directions of stage A and by the coverage report). */
int msspe_device_put(msspe_ctx *ctx, const void *host, size_t bytes, void **device_out);
/* The way back for such hosts: waits for the context's stream, then copies `bytes` bytes at `device` (from
 * msspe_device_put, or a device list a *_dev call filled) to host_out.  bytes == 0: MSSPE_OK, nothing read. */
int msspe_device_get(msspe_ctx *ctx, const void *device, size_t bytes, void *host_out);
/* The same for a matrix given as separate rows (an alignment held as one string per record): row r is
 * rows[r][0 .. row_bytes[r]) followed by `pad` bytes up to row_len; staged through pinned buffers, the
 * host never builds the rectangular copy. */
int msspe_device_put_rows(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                          size_t row_len, int pad, void **device_out);
/* The alignment in its compact device form: 2-bit bases + 1 validity bit per column (SURVEY.md 2.2, 8f-3;
 * replaces the per-window char vectors of od-msspe/src/main.rs:163-235).  A packed row is
 * msspe_packed_row_words(row_len) uint64: first (row_len + 31) / 32 words of bases (A 0, C 1, G 2, T 3; column
 * c in bits [2 (c % 32), +1] of word c / 32), then (row_len + 63) / 64 words of validity bits (1 = A / C / G / T;
 * '-', N, IUPAC codes and the padding of short rows are 0, which invalidates every k-mer that covers them,
 * main.rs:167).  msspe_device_put_rows_packed uploads the rows 16 MB at a time and packs each chunk on the
 * device; the *_packed_dev entry points are msspe_kmer_candidates_dev / msspe_segment_coverage_dev on that form
 * (same outputs; 3/8 of the bytes resident and read). */
/* Diagnostics of the last msspe_kmer_candidates* call (engine-only): per winner, iteration << 8 | how the greedy
 * loop selected it -- 1 a partition's leader read off the counts, 2 a word with postings in several partitions,
 * 3 such a word after its key was re-computed, 4 after a walk over posting lists, 0 the all-words loop.
 * *n_out = number of winners (also when capacity is smaller). */
int msspe_kmer_trace(msspe_ctx *ctx, uint32_t *out, int capacity, int *n_out);
size_t msspe_packed_row_words(size_t seq_len);
int msspe_device_put_rows_packed(msspe_ctx *ctx, const char *const *rows, const size_t *row_bytes, int n_rows,
                                 size_t row_len, void **device_out);
int msspe_kmer_candidates_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, int direction,
                                     uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);
/* Both directions of one alignment in one call (the reference runs find_candidates_kmers twice, main.rs:673-690):
 * direction 0 on the context's stream, direction 1 on a second stream of the context from a second host thread -- each
 * direction is a chain of small dependent launches and host round trips, which overlap.  Same results as two
 * msspe_kmer_candidates_packed_dev calls; msspe_kmer_trace and the stage_a_* infos then describe direction 0. */
int msspe_kmer_candidates_both_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                          const msspe_kmer_opt *opt, uint64_t *words_fwd, uint32_t *freq_fwd, int *n_fwd,
                                          uint64_t *words_rev, uint32_t *freq_rev, int *n_rev, int capacity);
/* Stage A extending a panel (engine extension): the same calls, started from a state in which the seed words are
 * already picked.  seed: n_seed HOST packed words (msspe_pack_oligos at opt->kmer_size) in the key space of the
 * direction -- direction 0 the forward primer text, direction 1 the reverse primer as the CSV writes it (the word
 * stage A returns for direction 1).  Before the first iteration every distinct seed word present in the direction's
 * index gets main.rs:371-378's post-push update once: its segments become covered, and the coverage of each distinct
 * partition among all its segments (covered ones included) goes up by one.  Seed order and duplicates do not
 * matter; a seed absent from the index does nothing; seeds are never returned as winners.  The loop, its stop rules
 * and max_iterations are unchanged; frequencies are live counts.  n_seed == 0 gives the unseeded call's output.
 * MSSPE_ERR_ARG: seed == NULL with n_seed > 0, n_seed < 0, or a seed word with bits above 2 k. */
int msspe_kmer_candidates_seeded(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, int direction, const uint64_t *seed, int n_seed,
                                 uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);
int msspe_kmer_candidates_seeded_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                            const msspe_kmer_opt *opt, int direction, const uint64_t *seed,
                                            int n_seed, uint64_t *words_out, uint32_t *freq_out, int capacity,
                                            int *n_out);
/* Both directions, each seeded with its own list, each on its own stream (as msspe_kmer_candidates_both_packed_dev). */
int msspe_kmer_candidates_both_seeded_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                                 const msspe_kmer_opt *opt, const uint64_t *seed_fwd, int n_fwd_seed,
                                                 const uint64_t *seed_rev, int n_rev_seed, uint64_t *words_fwd,
                                                 uint32_t *freq_fwd, int *n_fwd, uint64_t *words_rev,
                                                 uint32_t *freq_rev, int *n_rev, int capacity);
/* Stage A with words it must never pick (engine extension; the other half of repairing a panel: keep what passed
 * the later filters, ban what failed, let the greedy loop fill the holes).  An EXCLUDED word is treated as if it
 * occurred in no search window of the direction: it is taken out of every window's k-mer list before the index is
 * built, so it has no postings and no count, is in no segment's word list, and can be neither a winner nor a seed.
 * Every other word keeps its own occurrences (masking the alignment would also take the overlapping k-mers), and the
 * first-occurrence rule per window (main.rs:168) is not affected.  exclude: n_exclude HOST packed words in the
 * direction's key space, exactly as seeds are given; order and duplicates do not matter, a word absent from the
 * index does nothing, a word in both lists is excluded (the seed is then absent).  n_exclude == 0 is the seeded call
 * bit for bit, launch for launch; both lists empty (or sets == NULL) is the unseeded call.  When everything is
 * excluded the call returns MSSPE_OK with *n_out = 0.  The loop, its stop rules, the frequencies (live counts) and
 * max_iterations are unchanged.  MSSPE_ERR_ARG: a NULL list with a positive count, a negative count, or a word
 * with bits above 2 k in either list; the context stays usable.  Everything else as the seeded siblings. */
typedef struct {
    const uint64_t *seed;    int n_seed;      /* as msspe_kmer_candidates_seeded */
    const uint64_t *exclude; int n_exclude;   /* HOST packed words, the direction's key space */
} msspe_kmer_sets;
int msspe_kmer_candidates_sets(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                               uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);
int msspe_kmer_candidates_sets_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                          const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                          uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out);
int msspe_kmer_candidates_both_sets_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                               const msspe_kmer_opt *opt, const msspe_kmer_sets *fwd,
                                               const msspe_kmer_sets *rev, uint64_t *words_fwd, uint32_t *freq_fwd,
                                               int *n_fwd, uint64_t *words_rev, uint32_t *freq_rev, int *n_rev,
                                               int capacity);
/* Stage A extending a panel on what the panel COVERS (engine extension).  A TOLERANT SEEDED run is a seeded run in
 * which "the seed's segments" are no longer the word's own postings but the segments of the direction in which the
 * seed word has a match under msspe_segment_coverage_mm*'s rule (mode 0), or a STABLE match under
 * msspe_segment_coverage_thal*'s rule (mode 1 ANY, mode 2 END1: stable iff t_match > msspe_t_cut(tm_threshold)).
 *   - The match rule is applied with that direction's primers only: direction 0 the forward words in the head window,
 *     direction 1 the reverse word as the CSV writes it, in the tail window against the reverse-complemented candidate.
 *   - Before the first iteration every distinct seed word gets main.rs:371-378's post-push update once over that
 *     segment set: its segments become ignored, and coverage[j] goes up by one for every distinct partition j among ALL
 *     its segments, those already covered included.  The updates commute: seed order and duplicates do not matter.
 *   - A seed that is absent from the index may still cover segments.
 *   - The loop, its stop rules, max_iterations, the frequencies (live counts) and the winners' pushes are unchanged: a
 *     winner still covers its own postings only.  Seeds are never returned as winners (their exact postings are a
 *     subset of what they cover).
 *   - Exclusions act on the index as in msspe_kmer_candidates_sets*; they do not change what a seed covers (a panel
 *     primer is in the tube whether or not stage A may pick it).
 * Outputs per direction next to the _sets call's, both optional (NULL: not read back): seed_covered_out (HOST, n_seq * P
 * bytes, s = r * P + j): 1 where the segment is ignored before the first iteration; seed_partitions_out (HOST,
 * uint32[P]): coverage[] at that moment.  Both are zeros when there is no seed.
 * Identities: n_seed == 0 is the _sets call, bit for bit and launch for launch.  Mode 0 with max_mismatches 0, any
 * exact_3p and no word in both lists gives the _sets call's winners and frequencies.  Mode 1 / 2 with tm_threshold
 * <= 0 gives mode 0.  seed_covered_out == (best_out != 255) of msspe_segment_coverage_mm* called with that direction's
 * seeds alone, and in modes 1 and 2 == (held_out == 2) of msspe_segment_coverage_thal*.
 * The incidence is built in TILES OF SEEDS, each against all segment groups, in the matrix of msspe_panel_thin* (the
 * state is an OR and a sum over seeds); a tile is as many seeds (a multiple of 64) as "panel_thin_matrix_max_mb" holds,
 * and MSSPE_ERR_CAPACITY is returned only when 64 seeds do not fit.  Modes 1 and 2 list, score and fold a tile as
 * msspe_panel_thin_thal* does ("thin_thal_unique", "site_list_cap_log2" and its overrun rule apply).  The both call
 * runs the two seeding passes one after the other on the context's stream; the two greedy loops overlap as before.
 * msspe_get_info, the last call (both directions added up): "stage_a_tolerant_tiles", "stage_a_tolerant_segments"
 * (segments the seeds covered), "stage_a_tolerant_incidence_us" / "stage_a_tolerant_seed_us" (device time filling the
 * matrix / seeding from it).
 * Errors: those of the _sets calls, of msspe_segment_coverage_mm* (max_mismatches or exact_3p outside 0..k) and, in
 * modes 1 and 2, of msspe_segment_coverage_thal* (MSSPE_ERR_K below k = 2); MSSPE_ERR_ARG: rule == NULL, a mode
 * outside 0..2, chem == NULL in mode 1 or 2.  Out of scope: winners that cover tolerantly, seeds of another length
 * than kmer_size. */
typedef struct {
    int max_mismatches, exact_3p;   /* as msspe_mismatch_opt */
    int mode;                       /* 0: a match covers; 1 ANY / 2 END1: a STABLE match covers */
    const msspe_chem *chem;         /* mode 1, 2 */
    float tm_threshold;             /* mode 1, 2: stable iff t_match > msspe_t_cut(tm_threshold) */
} msspe_seed_rule;
int msspe_kmer_candidates_tolerant(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                   const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                   const msspe_seed_rule *rule, uint64_t *words_out, uint32_t *freq_out, int capacity,
                                   int *n_out, uint8_t *seed_covered_out, uint32_t *seed_partitions_out);
int msspe_kmer_candidates_tolerant_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                              const msspe_kmer_opt *opt, int direction, const msspe_kmer_sets *sets,
                                              const msspe_seed_rule *rule, uint64_t *words_out, uint32_t *freq_out,
                                              int capacity, int *n_out, uint8_t *seed_covered_out,
                                              uint32_t *seed_partitions_out);
int msspe_kmer_candidates_both_tolerant_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                                   const msspe_kmer_opt *opt, const msspe_kmer_sets *fwd,
                                                   const msspe_kmer_sets *rev, const msspe_seed_rule *rule,
                                                   uint64_t *words_fwd, uint32_t *freq_fwd, int *n_fwd,
                                                   uint64_t *words_rev, uint32_t *freq_rev, int *n_rev, int capacity,
                                                   uint8_t *seed_covered_fwd, uint32_t *seed_partitions_fwd,
                                                   uint8_t *seed_covered_rev, uint32_t *seed_partitions_rev);
int msspe_segment_coverage_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                      const msspe_kmer_opt *opt, const uint64_t *fwd_words, int n_fwd,
                                      const uint64_t *rev_words, int n_rev, uint8_t *hit_out);
int msspe_device_free(msspe_ctx *ctx, void *device);

/* ---- coverage within N mismatches, the primer's 3' end exact (engine extension, no reference counterpart) ----
 * Generalises the exact rule of coverage_report() (od-msspe/src/main.rs:518-594, msspe_segment_coverage*): the same
 * segments (record r, partition j, P = (seq_len - segment_size) / overlap_size + 1) and windows.  For each position p
 * in [0, W - k] (W = search_window_size, k = kmer_size, 1 <= k <= 31) the FORWARD candidate is the k bases of the head
 * window at p, the REVERSE candidate the reverse complement of the k bases of the tail window at p.  A position that
 * holds any base other than A / C / G / T ('-', N, IUPAC codes) is never a match, at any max_mismatches (main.rs:167;
 * a gap column is not a base, so it is not a mismatch either).  A candidate w matches a primer word u of its direction
 * (fwd_words / rev_words: msspe_pack_oligos form, a reverse word in primer orientation as the CSV writes it) when
 *   - the number of base positions q in [0, k) where w and u differ is <= max_mismatches, and
 *   - they agree at every q in [k - exact_3p, k): the primer's last exact_3p bases (its 3' end) match.
 * best_out[r * P + j] (host, n_seq * P bytes): the smallest mismatch count over all matches in the segment, either
 * direction; 255 when there is none.  primer_segments_out (host, optional, n_fwd + n_rev: forward primers first, then
 * reverse, in the caller's order): the number of segments whose head (forward) / tail (reverse) window holds at least
 * one match of that primer; duplicates are counted independently.  NULL: that work is not done.
 * At max_mismatches 0, best_out == 0 exactly where msspe_segment_coverage's hit_out is 1, for every exact_3p.
 * MSSPE_ERR_ARG: mm, best_out, or a primer list with a nonzero count NULL; max_mismatches or exact_3p outside 0..k;
 * a primer word with bits above 2 k; window, segment or stride as msspe_segment_coverage.  MSSPE_ERR_K: k outside
 * 1..31.  No segments: MSSPE_OK with primer_segments_out zeroed.  The *_dev / *_packed_dev forms read the alignment
 * from the device (bytes as msspe_segment_coverage_dev, packed rows as msspe_device_put_rows_packed makes them). */
typedef struct {
    int max_mismatches;   /* 0 .. kmer_size */
    int exact_3p;         /* 0 .. kmer_size: the primer's last exact_3p bases must match */
} msspe_mismatch_opt;

int msspe_segment_coverage_mm(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              uint8_t *best_out, uint32_t *primer_segments_out);
int msspe_segment_coverage_mm_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  uint8_t *best_out, uint32_t *primer_segments_out);
int msspe_segment_coverage_mm_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                         const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                         const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                         uint8_t *best_out, uint32_t *primer_segments_out);

/* ---- a panel thinned to the primers its coverage needs (engine extension, no reference counterpart) ----------
 * Stage A picks words by exact occurrence, so two words that differ at one 5' base are both picked although either
 * primes both variants.  This call answers "which of these primers could I leave out without losing a segment?" by
 * a greedy set cover over the incidence of msspe_segment_coverage_mm*: the alignment, msspe_kmer_opt,
 * msspe_mismatch_opt and primer words are that call's, and I[p][s] = 1 when primer p has at least one match in segment
 * s under exactly its rule (a forward primer in the head window, a reverse primer in the tail window against the
 * reverse-complemented candidate).  p runs over the forward primers in the caller's order, then the reverse primers;
 * n = n_fwd + n_rev; s = r * P + j.  A row sum of I is that call's primer_segments_out[p].
 *   forced (host, optional, n bytes; NULL: none): forced[p] != 0 keeps primer p whatever it covers (a panel being
 *     extended).  covered starts as the OR of the forced rows; a forced primer is never picked and never in the order.
 *   Rounds: for every p neither forced nor picked, gain(p) = |{s : I[p][s] and not covered[s]}|.  The round picks the p
 *     of greatest gain, ties to the LOWEST index.  If that gain is below thin->min_gain the loop ends; otherwise p is
 *     appended to the order with its gain and covered |= I[p].  (A duplicate of a picked word has gain 0.)
 *   keep_out[n]: 1 when forced or picked.  order_out / gain_out (the caller sizes both to n) and *n_picked_out: the
 *     picks in order with their gains.  covered_out (optional, n_seq * P bytes): 1 where the kept set covers.
 *     *covered_all_out (optional): segments the whole set covers, |OR of all I[p]|; *covered_kept_out (optional): the
 *     kept set's.
 * GUARANTEE: at min_gain 1 the two counts are equal and covered_out marks exactly the segments where the whole set's
 * msspe_segment_coverage_mm best_out != 255 -- thinning loses no segment.  What it does NOT preserve is the smallest
 * mismatch count per segment: a segment matched exactly before may be matched with up to max_mismatches mismatches
 * afterwards.  Choose max_mismatches and exact_3p for the thinning on their own, separately from a report's.
 * The incidence matrix takes ceil(n_seq * P / S) * ceil(n / 64) * 512 bytes in the context (S <= 64 segments per
 * group: 53 at window 50, k 13); msspe_set_option "panel_thin_matrix_max_mb" (default 8192) bounds it, and a call that
 * needs more returns MSSPE_ERR_CAPACITY with both figures in msspe_last_error: it never thins on part of the data.
 * Errors: those of msspe_segment_coverage_mm*, and MSSPE_ERR_ARG for thin == NULL, min_gain < 1, or a NULL keep_out,
 * order_out, gain_out or n_picked_out.  n == 0 or no segments: MSSPE_OK, nothing picked, both counts 0, keep_out = the
 * forced flags.  msspe_get_info "panel_thin_rounds" / "panel_thin_groups" / "panel_thin_*_us" describe the last call. */
typedef struct {
    int min_gain;   /* >= 1: a pick must cover at least this many segments nothing kept covers yet */
} msspe_thin_opt;

int msspe_panel_thin(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                     const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                     const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                     uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                     long long *covered_all_out, long long *covered_kept_out);
int msspe_panel_thin_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                         const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                         const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                         uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                         long long *covered_all_out, long long *covered_kept_out);
int msspe_panel_thin_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                                long long *covered_kept_out);

/* ---- off-target sites in a background (engine extension, no reference counterpart) --------------------------
 * Where else do the primers land: a host genome, rRNA, a mitochondrion.  The BACKGROUND is a list of records
 * (unaligned, of any lengths, empty ones allowed) seen as one STREAM: the records back to back with one invalid
 * column between two records; record r starts at stream column start[r] = start[r - 1] + record_bytes[r - 1] + 1,
 * start[0] = 0, and the stream is total_len = start[n_records - 1] + record_bytes[n_records - 1] columns long (0
 * without records); total_len < 2^32.  Only upper-case A C G T are bases; every other byte (N, IUPAC codes, '-',
 * lower case, the separator) is invalid, as in msspe_device_put_rows_packed -- a caller that wants lower case or U
 * taken as bases normalises first.
 * For every stream position p in [0, total_len - k] and every primer word u (words: n HOST words in
 * msspe_pack_oligos form, primer orientation, the way the CSV writes forward and reverse primers alike; 1 <= k <= 31):
 *   - PLUS-strand site: the k columns at p are all bases and, read as a word w, match u by the rule of
 *     msspe_mismatch_opt: at most max_mismatches differing base positions, and equal on u's last exact_3p bases;
 *   - MINUS-strand site: the same test with w = the reverse complement of the k columns at p.
 * A window that holds an invalid column is never a site, so no site straddles two records.  Every primer is tested
 * on both strands whatever its direction; a position can be a site on both strands for one primer (palindromes)
 * and then counts twice.
 * sites_out[2 * i + s] (uint64, HOST, 2 n): the sites of primer i on strand s (0 plus, 1 minus); duplicate primers
 * are counted independently.  The optional SITE LIST follows the edge list's convention
 * (msspe_cross_dimer_edges*): one msspe_site per site, appended with one atomic each in no particular order,
 * capacity and count owned by the caller (the _packed_dev form adds to *d_count, which the caller zeroes; it keeps
 * running past the capacity, so a truncated list is visible and nothing is written behind d_sites[capacity - 1]).
 * pos is the stream position p; with record_start_out it becomes (record, offset).
 *   msspe_device_put_stream_packed: uploads the records 16 MB at a time through pinned staging and packs each
 *     chunk on the device into ONE packed row of msspe_packed_row_words(total_len) words (the host never builds the
 *     concatenated copy).  record_start_out (optional, n_records): start[].  Free with msspe_device_free.
 *   msspe_background_sites_packed_dev: the kernel call on a resident stream, on the context's stream; d_sites ==
 *     NULL: no list (capacity and d_count are not read).  Work buffers grow on first use and are kept; the call
 *     returns when sites_out is filled.
 *   msspe_background_sites: host pointers throughout.  sites == NULL: no list.  Otherwise the first `capacity`
 *     records to arrive, sorted by (primer, strand, pos), *count_out = the number of sites; when that exceeds
 *     `capacity` the call returns MSSPE_ERR_CAPACITY (sites_out and count_out are valid: retry with count_out).
 * MSSPE_ERR_ARG: mm, sites_out, words with n > 0, records with n_records > 0, or count_out with a list NULL;
 * max_mismatches or exact_3p outside 0..k; a primer word with bits above 2 k; total_len >= 2^32.  MSSPE_ERR_K: k
 * outside 1..31.  n == 0 or total_len < k: MSSPE_OK, sites_out zeroed, list count 0 (_packed_dev: unchanged). */
typedef struct {
    uint32_t primer;       /* index into words */
    uint32_t pos;          /* stream position of the window's first column */
    uint16_t mismatches;   /* differing base positions, 0 .. max_mismatches */
    uint16_t strand;       /* 0 plus, 1 minus */
} msspe_site;
int msspe_device_put_stream_packed(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                   int n_records, void **device_out, size_t *total_len_out,
                                   uint64_t *record_start_out);
int msspe_background_sites_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                      const msspe_mismatch_opt *mm, const uint64_t *words, int n, uint64_t *sites_out,
                                      msspe_site *d_sites, uint64_t capacity, uint64_t *d_count);
int msspe_background_sites(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                           int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, uint64_t *sites_out,
                           msspe_site *sites, uint64_t capacity, uint64_t *count_out, uint64_t *record_start_out);

/* ---- thal score of every background site (engine extension) --------------------------------------------------
 * msspe_background_sites* says where a primer lands by a string rule; these calls say which of those sites would
 * hold the primer.  Take a site {primer u, pos p, strand s} of the rule above and let w be the k columns at p.  The
 * TEMPLATE OLIGO o2 is the strand the primer anneals to, written 5'->3':
 *   strand 0 (plus):  o2 = revcomp(w);
 *   strand 1 (minus): o2 = w  (the near-copy of u there is revcomp(w), whose partner strand is w itself).
 * Both oligos are k bases long, and an exact site gives o2 = revcomp(u) on either strand.  Bases beyond the window
 * (dangling ends) are not part of the score; msspe_background_thal_flank* below adds them.
 * The SITE SCORE is thal of (oligo 1 = u, oligo 2 = o2) under chem; mode is 1 for ANY and 2 for END1, the numbering of
 * msspe_thal_detail_pairs (END1: structures that close on the primer's 3' base, the ones that can prime).  Raw dG is
 * +inf without a structure and raw t is 0 without one.  t_site = max(0, t), and a site is STABLE iff
 * !(msspe_round_fixed_f32(t_site, 2) < tm_threshold), which the kernels test as t_site > msspe_t_cut(tm_threshold):
 * the END screen's rule and stage B's.  A threshold <= 0 makes every site stable.
 *   sites_out[2 i + s]  (uint64, HOST, 2 n): as msspe_background_sites_packed_dev returns for the same arguments.
 *   stable_out[2 i + s] (uint64, HOST, 2 n): the stable sites of primer i on strand s, exact however many sites
 *     there are.
 *   The optional list follows the edge list's convention: one msspe_scored_site per SITE, stable or not, dg and t raw,
 *     in no particular order; capacity and count are the caller's (the _packed_dev form adds to *d_count, which the
 *     caller zeroes and which runs past the capacity; nothing is written behind d_sites[capacity - 1]).  The host form
 *     sorts by (primer, strand, pos) and returns MSSPE_ERR_CAPACITY with a valid count, as msspe_background_sites.
 * Memory is bounded and nothing is dropped: the scores pass through a work list of 2^site_list_cap_log2 sites in
 * the context (msspe_set_option "site_list_cap_log2", 12..26, default 22: 44 bytes per entry; msspe_get_info reports
 * it).  The stream is worked through in slabs of runs of 2048 positions; a slab whose sites exceed the work list
 * -- the site kernel's counter runs past the capacity -- is split and done again (runs first, then primers: one
 * run against one primer has at most 4096 sites), and no count ever comes from a truncated list.  msspe_get_info
 * "background_thal_slabs" / "background_thal_redone": slabs scored / slabs split by the last call.
 * Routing is the END screen's, over the explicit pair list: k <= 16 with a chemistry the register-table kernels take
 * and max_loop >= 2 k - 4: the 56-slot list kernel, the 72-slot one, one wave per pair, the dense kernel; otherwise
 * one wave per pair, then the dense kernel.  Options force_generic, wave_kernel and list_cap_log2 apply as there.
 * Errors: the statuses of msspe_background_sites*; MSSPE_ERR_K for k outside 2..31 (thal needs two bases);
 * MSSPE_ERR_ARG for a NULL chem or stable_out or a mode outside {1, 2}.  n == 0 or total_len < k: MSSPE_OK, outputs
 * zeroed, list count 0 (_packed_dev: unchanged). */
typedef struct {
    uint32_t primer;       /* index into words */
    uint32_t pos;          /* stream position of the window's first column */
    uint16_t mismatches;   /* differing base positions, 0 .. max_mismatches */
    uint16_t strand;       /* 0 plus, 1 minus */
    uint32_t stable;       /* 1 iff max(0, t) > msspe_t_cut(tm_threshold) */
    double dg;             /* raw dG, +inf without a structure */
    double t;              /* raw t, 0 without a structure */
} msspe_scored_site;
int msspe_background_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                     const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                     const msspe_chem *chem, int mode, float tm_threshold, uint64_t *sites_out,
                                     uint64_t *stable_out, msspe_scored_site *d_sites, uint64_t capacity,
                                     uint64_t *d_count);
int msspe_background_thal(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                          int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                          int mode, float tm_threshold, uint64_t *sites_out, uint64_t *stable_out,
                          msspe_scored_site *sites, uint64_t capacity, uint64_t *count_out,
                          uint64_t *record_start_out);

/* ---- the same score with template flanks: dangling ends (engine extension) -----------------------------------
 * A real template does not stop at the window: the bases next to it stack on the duplex ends (dangling ends, terminal
 * mismatches) and let thal find shifted or bulged alignments, which is how Primer3 scores template mispriming.  Each
 * call below is its sibling above with one argument, flank = f, after tm_threshold; 0 <= f <= 4 and k + 2 f <= 32.
 * Take a site {primer u, pos p, strand s}; sites, mismatch counts and sites_out do not depend on the flank.
 *   fl = the consecutive base columns (upper-case A C G T) that end at column p - 1, at most f;
 *   fr = the consecutive base columns that start at column p + k, at most f.
 * An invalid column stops the count: N, IUPAC codes, lower case, '-', the separator between two records and the ends
 * of the stream.  A flank therefore never crosses a record boundary and the template oligo is pure ACGT.
 *   The EXTENDED WINDOW is W = stream[p - fl, p + k + fr); o2 = revcomp(W) on the plus strand and W on the minus
 *   strand, k + fl + fr bases; the site score is thal of (oligo 1 = u, oligo 2 = o2), mode and chemistry as above.
 * t_site, the stable rule and msspe_t_cut are unchanged, and f = 0 is exactly the definition above: the calls without
 * _flank are the f = 0 case of the same pass, bit for bit.  Records, lists, counts, sorting, the capacity contract,
 * the work list and its slabs are the siblings'; msspe_scored_site is unchanged.
 * Routing: the sites of a work-list chunk are grouped by class (fl, fr) on the device, and every non-empty class is
 * scored as one explicit pair list with template length k + fl + fr.  Class (0, 0) -- the only one at f = 0 -- takes
 * the routing described above; every other class is a rectangle and runs one wave per pair where the wave kernel takes
 * the template's length, then the dense kernel.  Options force_generic, wave_kernel, list_cap_log2 and
 * site_list_cap_log2 apply as above.  At f = 0 no additional kernel runs.  msspe_get_info
 * "background_thal_flank_classes" / "background_thal_truncated": classes scored by the last call / sites with fl < f
 * or fr < f.
 * Errors: MSSPE_ERR_ARG for a flank outside 0..4 or k + 2 flank > 32; everything else as the siblings. */
int msspe_background_thal_flank_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                           const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                           const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                           uint64_t *sites_out, uint64_t *stable_out, msspe_scored_site *d_sites,
                                           uint64_t capacity, uint64_t *d_count);
int msspe_background_thal_flank(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                int n_records, int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                const msspe_chem *chem, int mode, float tm_threshold, int flank, uint64_t *sites_out,
                                uint64_t *stable_out, msspe_scored_site *sites, uint64_t capacity,
                                uint64_t *count_out, uint64_t *record_start_out);

/* ---- off-target amplicons from the stable sites (engine extension) ---------------------------------------------
 * One stable off-target site costs a little primer; two that face each other within a few hundred bases amplify the
 * background.  Take the stream, primers, msspe_mismatch_opt, chemistry, mode and tm_threshold of
 * msspe_background_thal* and its STABLE sites as defined there (a threshold <= 0: every site of the string rule).
 * A primer at a plus-strand site at stream position p extends towards increasing positions, one at a minus-strand
 * site at q towards decreasing positions.  An AMPLICON is an ordered pair of stable sites -- a plus-strand site of
 * primer `fwd` at p and a minus-strand site of primer `rev` at q -- with
 *   - q >= p;
 *   - len = q + k - p in [min_len, max_len] (the product's length, both primers included);
 *   - both windows in the same record: start[r] <= p and q + k <= start[r] + record_bytes[r] for one r.  Invalid
 *     columns inside a record (N, IUPAC) between the two sites do not break an amplicon; the separator between two
 *     records does.
 * fwd == rev is allowed (one primer priming both ends); q == p is allowed (a palindromic window that is a site on
 * both strands, len = k); duplicate primers count independently; every (plus site, minus site) pair that qualifies
 * is one amplicon.
 *   sites_out, stable_out: exactly what msspe_background_thal* returns for the same arguments.
 *   amplicons_out (uint64, HOST, 2 n): [2 i] the amplicons with primer i as fwd, [2 i + 1] as rev.
 *   *n_amplicons_out: the number of amplicons (the sum of either column).
 *   The optional list follows the edge list's convention: one msspe_amplicon per amplicon; the _packed_dev form adds
 *     to *d_count, which the caller zeroes and which runs past the capacity; nothing is written behind
 *     d_amplicons[capacity - 1] and the order is unspecified (d_amplicons == NULL: no list, capacity and d_count
 *     are not read).  The host form sorts by (pos, len, fwd, rev) and returns MSSPE_ERR_CAPACITY with valid counts
 *     and *count_out = the number of amplicons when the list is truncated.  Counts never come from a truncated list.
 *   record_start (HOST, n_records, the _packed_dev form): start[] as msspe_device_put_stream_packed returns it,
 *     start[0] == 0; NULL: the stream is one record (n_records is not read).  The host form fills record_start_out (optional).
 * Memory is bounded and nothing is dropped: the scored pass appends one 64-bit key per stable site to a buffer in the
 * context that starts at 2^amplicon_keys_cap_log2 keys (msspe_set_option, 10..28, default 20) and doubles -- before a
 * slab is folded it has room for the keys so far plus every site of the slab; a grown buffer is kept for later calls.  The keys are sorted by position
 * (rocPRIM) and joined on the device; msspe_get_info "amplicon_keys" / "amplicon_key_grows": stable keys of the last
 * call / doublings.  Primers of one call have one length; a panel of mixed lengths is one call per length and pairs
 * no primers across them.
 * Errors: those of msspe_background_thal*; MSSPE_ERR_ARG also for a NULL amp, amplicons_out or n_amplicons_out,
 * min_len < k, min_len > max_len, record_start[0] != 0, record_start not strictly ascending or its last start beyond
 * total_len; MSSPE_ERR_NOMEM for 2^31 stable sites or more.  n == 0 or
 * total_len < k: MSSPE_OK, outputs zeroed, list count 0 (_packed_dev: unchanged). */
typedef struct {
    uint32_t min_len, max_len;   /* k <= min_len <= max_len */
} msspe_amplicon_opt;
typedef struct {
    uint32_t fwd, rev;     /* indices into words: the plus-strand site's primer, the minus-strand site's */
    uint32_t pos;          /* p: stream position of the plus-strand site's first column */
    uint32_t len;          /* q + k - p */
} msspe_amplicon;
int msspe_background_amplicons_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                          const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                          const msspe_chem *chem, int mode, float tm_threshold,
                                          const msspe_amplicon_opt *amp, const uint64_t *record_start, int n_records,
                                          uint64_t *sites_out, uint64_t *stable_out, uint64_t *amplicons_out,
                                          uint64_t *n_amplicons_out, msspe_amplicon *d_amplicons, uint64_t capacity,
                                          uint64_t *d_count);
int msspe_background_amplicons(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                               int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                               const msspe_chem *chem, int mode, float tm_threshold, const msspe_amplicon_opt *amp,
                               uint64_t *sites_out, uint64_t *stable_out, uint64_t *amplicons_out,
                               uint64_t *n_amplicons_out, msspe_amplicon *amplicons, uint64_t capacity,
                               uint64_t *count_out, uint64_t *record_start_out);
/* The same with template flanks: the amplicons of the stable sites of msspe_background_thal_flank* (flank after
 * tm_threshold, 0..4, k + 2 flank <= 32).  len, pos and the same-record rule still refer to the k-column windows;
 * flank 0 is the two calls above. */
int msspe_background_amplicons_flank_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                                const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                                const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                                const msspe_amplicon_opt *amp, const uint64_t *record_start,
                                                int n_records, uint64_t *sites_out, uint64_t *stable_out,
                                                uint64_t *amplicons_out, uint64_t *n_amplicons_out,
                                                msspe_amplicon *d_amplicons, uint64_t capacity, uint64_t *d_count);
int msspe_background_amplicons_flank(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes,
                                     int n_records, int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                     const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                     const msspe_amplicon_opt *amp, uint64_t *sites_out, uint64_t *stable_out,
                                     uint64_t *amplicons_out, uint64_t *n_amplicons_out, msspe_amplicon *amplicons,
                                     uint64_t capacity, uint64_t *count_out, uint64_t *record_start_out);

/* ---- target reach: the columns each record's primers extend into (engine extension) ---------------------------
 * A spiked primer enriches what a polymerase extends from it, a few hundred bases downstream of its site.  These calls
 * say how much of every record of a stream lies within that distance of a stable site, and where the longest stretch
 * lies that nothing primes into.  The stream, records, start[], total_len, primers, msspe_mismatch_opt, chemistry, mode,
 * tm_threshold, flank and the STABLE sites are those of msspe_background_thal_flank* (a threshold <= 0: every site of
 * the string rule).  Record r spans the columns [s_r, e_r), s_r = start[r], e_r = s_r + record_bytes[r].
 *   P_r: the positions p of the stable plus-strand sites in r, of any primer; duplicate primers and several primers at
 *        one p count once.  M_r: the same set for the minus-strand sites q.
 *   The REACH D (msspe_reach_opt.reach) is the length of the extension product, the primer included: k <= D < 2^31.
 *   Column b of r is PLUS-REACHED  iff some p in P_r has p <= b <= p + D - 1;
 *                    MINUS-REACHED iff some q in M_r has q + k - D <= b <= q + k - 1 (a primer at a minus site extends
 *                    towards decreasing positions, as in the amplicon section).
 *   Reach never leaves its record.  Invalid columns inside a record (N, IUPAC) are columns like any other: they are
 *   counted and do not stop reach, just as they do not break an amplicon.
 * One msspe_reach_record per record:
 *   sites_plus, sites_minus: |P_r|, |M_r|;
 *   reached_plus, reached_minus, reached_either, reached_both: columns of r;
 *   gap_plus_len / gap_plus_pos, gap_minus_*, gap_either_*: the longest maximal run of columns of r that are not
 *     plus-reached / not minus-reached / reached on neither strand; pos is the stream position of the run's first
 *     column, ties go to the lowest position, and len = 0 gives pos = s_r.
 *   An empty record is all zeros with every pos = s_r.
 *   msspe_stream_reach_packed_dev: on a resident stream (msspe_device_put_stream_packed), on the context's stream.
 *     record_start (HOST, n_records) has the conventions of msspe_background_amplicons_packed_dev: start[] as
 *     msspe_device_put_stream_packed returns it, start[0] == 0, the column before every later start is the separator;
 *     NULL: the stream is one record (n_records is not read).  sites_out, stable_out (uint64, HOST, 2 n): exactly what
 *     msspe_background_thal_flank* returns for the same arguments.  records_out: HOST, n_records entries (one for
 *     NULL record_start).  The call returns when they are filled.
 *   msspe_stream_reach: host pointers throughout; record_start_out (optional, n_records): start[].
 * Memory is bounded and nothing depends on the number of sites: the scored pass ORs every stable site into one of two
 * bit planes of ceil(total_len / 64) words, a third plane holds "reached by neither", and the nearest site is carried
 * across tiles of "reach_tile_columns" columns through three 32-bit values per tile.  The buffers are the context's,
 * grown when a call needs more and kept.  msspe_get_info "reach_plane_bytes": the planes' size; "reach_grows": 1 when
 * the last call grew the planes, otherwise 0; "reach_tile_columns"; "reach_tiles_us", "reach_scan_us", "reach_masks_us",
 * "reach_gap_tiles_us", "reach_gaps_us": device time of the last call's reach kernels.
 * Errors: those of msspe_background_thal_flank*; MSSPE_ERR_ARG also for a NULL reach_opt or records_out, a reach
 * outside [k, 2^31), record_start[0] != 0, record_start not strictly ascending or its last start beyond total_len.
 * n == 0 or total_len < k: MSSPE_OK, sites_out and stable_out zeroed, and every record has no site and no reached
 * column: every gap is the whole record, len = record_bytes[r], pos = s_r. */
typedef struct {
    uint32_t reach;        /* D: k <= reach < 2^31 */
} msspe_reach_opt;
typedef struct {
    uint32_t sites_plus, sites_minus;
    uint32_t reached_plus, reached_minus, reached_either, reached_both;
    uint32_t gap_plus_len, gap_plus_pos;
    uint32_t gap_minus_len, gap_minus_pos;
    uint32_t gap_either_len, gap_either_pos;
} msspe_reach_record;
int msspe_stream_reach_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                  const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                                  int mode, float tm_threshold, int flank, const msspe_reach_opt *reach_opt,
                                  const uint64_t *record_start, int n_records, uint64_t *sites_out,
                                  uint64_t *stable_out, msspe_reach_record *records_out);
int msspe_stream_reach(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records, int k,
                       const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem, int mode,
                       float tm_threshold, int flank, const msspe_reach_opt *reach_opt, uint64_t *sites_out,
                       uint64_t *stable_out, msspe_reach_record *records_out, uint64_t *record_start_out);

/* ---- a panel thinned on target reach: the primers the reach needs (engine extension) --------------------------
 * msspe_stream_reach* says which columns a panel reaches; these calls say which of its primers are needed to reach
 * them, by a greedy set cover over COLUMNS.  The stream, records, start[], total_len, k, msspe_mismatch_opt, words / n,
 * chemistry, mode, tm_threshold, flank, msspe_reach_opt and the stable sites are those of msspe_stream_reach*;
 * msspe_thin_opt, forced, keep_out, order_out, gain_out and *n_picked_out follow msspe_panel_thin*.
 *   R_p: the columns primer p reaches on either strand -- the union, over the stable sites of p alone, of
 *        [p_pos, min(p_pos + D, e_r) - 1] for a plus site at p_pos and [max(q + k - D, s_r), q + k - 1] for a minus site
 *        at q, r the site's record.  Reach never leaves the site's record.  A word listed twice has two equal sets.
 *   forced (host, optional, n bytes; NULL: none): C starts as the union of the forced primers' sets; a forced primer is
 *        never picked and never in the order.
 *   Rounds: the round picks the unforced, unpicked p with the greatest |R_p \ C|, ties to the LOWEST index.  If that
 *        gain is below thin->min_gain the loop ends; otherwise p is appended to the order with its gain and C |= R_p.
 *   keep_out[n]: 1 when forced or picked.  order_out / gain_out (the caller sizes both to n) and *n_picked_out: the
 *        picks in order, each with its gain at the time of the pick.
 *   reach_out[n] (optional): |R_p|, each primer's own reach, whatever is forced.
 *   *reached_all_out, *reached_kept_out (optional): |union of R_p| over all primers and over the kept primers.
 *   sites_out, stable_out (uint64, HOST, 2 n): as msspe_stream_reach*, for the WHOLE panel.
 *   records_out (optional, NULL skips it; HOST, n_records entries, one for NULL record_start): one msspe_reach_record
 *        per record for the KEPT panel.  It equals msspe_stream_reach* called on the kept words alone -- stability is
 *        a property of (primer, template) -- and is built from the kept primers' sites of this call's scored pass:
 *        no second pass runs.
 *   msspe_panel_thin_reach_packed_dev: on a resident stream, on the context's stream; record_start as there.
 *   msspe_panel_thin_reach: host pointers throughout; record_start_out (optional, n_records): start[].
 * GUARANTEE: at min_gain 1, reached_kept == reached_all, and records_out[r].reached_either equals that of
 * msspe_stream_reach* on the whole panel for every r -- thinning loses no reached column.  NOT preserved:
 * reached_plus, reached_minus and reached_both, the per-strand gaps, and the site counts.
 * Memory depends on the number of stable sites, as msspe_background_amplicons* does: the scored pass collects one key
 * per stable site in that call's buffer ("amplicon_keys_cap_log2" and its doubling), and the cover keeps about 60 bytes
 * per key (the sorted intervals) beside the planes of msspe_stream_reach* and 4 bytes per 64 columns.  2^31 stable
 * sites or more: MSSPE_ERR_NOMEM.  msspe_get_info, of the last call: "thin_reach_sites" (stable keys),
 * "thin_reach_intervals" (the disjoint intervals they leave), "thin_reach_rounds" (the picks and the round that
 * stopped), "thin_reach_prepare_us", "thin_reach_gain0_us", "thin_reach_rounds_us", "thin_reach_report_us" (device
 * time behind the scored pass: intervals; |R_p|, forced and first gains; rounds; counts and records).
 * Errors: those of msspe_stream_reach* (a NULL records_out is none here); MSSPE_ERR_ARG for a NULL thin, min_gain < 1,
 * or a NULL keep_out, order_out, gain_out or n_picked_out.  n == 0 or total_len < k: MSSPE_OK, nothing picked,
 * keep_out = the forced flags, both counts 0, and records_out as there: every gap is the whole record. */
int msspe_panel_thin_reach_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, size_t total_len, int k,
                                      const msspe_mismatch_opt *mm, const uint64_t *words, int n,
                                      const msspe_chem *chem, int mode, float tm_threshold, int flank,
                                      const msspe_reach_opt *reach_opt, const msspe_thin_opt *thin,
                                      const uint8_t *forced, const uint64_t *record_start, int n_records,
                                      uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                      uint32_t *reach_out, long long *reached_all_out, long long *reached_kept_out,
                                      uint64_t *sites_out, uint64_t *stable_out, msspe_reach_record *records_out);
int msspe_panel_thin_reach(msspe_ctx *ctx, const char *const *records, const size_t *record_bytes, int n_records,
                           int k, const msspe_mismatch_opt *mm, const uint64_t *words, int n, const msspe_chem *chem,
                           int mode, float tm_threshold, int flank, const msspe_reach_opt *reach_opt,
                           const msspe_thin_opt *thin, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out,
                           uint32_t *gain_out, int *n_picked_out, uint32_t *reach_out, long long *reached_all_out,
                           long long *reached_kept_out, uint64_t *sites_out, uint64_t *stable_out,
                           msspe_reach_record *records_out, uint64_t *record_start_out);

/* ---- segment coverage scored with thal (engine extension, no reference counterpart) ---------------------------
 * msspe_segment_coverage_mm* says which segments hold a match by a string rule; these calls say which of those
 * matches would hold the primer at a temperature -- msspe_background_thal*'s question, asked of the target alignment.
 * The alignment, msspe_kmer_opt, msspe_mismatch_opt and primer words (HOST, msspe_pack_oligos form, a reverse word in
 * primer orientation) are those of msspe_segment_coverage_mm*, and so are segments, windows, positions and validity.
 * A MATCH is a triple (segment s = r * P + j, primer index q, window position p) that rule accepts; q runs over the
 * forward primers first, then the reverse primers.  A forward primer is compared in the head window, a reverse primer
 * against the reverse complement of the tail window's k columns.  The TEMPLATE OLIGO o2 is the strand the primer
 * anneals to, written 5'->3':
 *   forward primer: o2 = revcomp(the head window's k columns at p);
 *   reverse primer: o2 = the tail window's k columns at p, as written.
 * These are the plus- and minus-strand rules of msspe_background_thal*; an exact match gives o2 = revcomp(u) in either
 * direction.  The MATCH SCORE is thal of (oligo 1 = u, oligo 2 = o2) under chem; mode is 1 for ANY and 2 for END1, the
 * numbering of msspe_thal_detail_pairs.  Raw dG is +inf and raw t is 0 without a structure.  t_match = max(0, t), and
 * the match is STABLE iff !(msspe_round_fixed_f32(t_match, 2) < tm_threshold), which the kernels test as
 * t_match > msspe_t_cut(tm_threshold): the END screen's, stage B's and msspe_background_thal*'s rule.  A threshold
 * <= 0 makes every match stable.  Template bases beyond the k columns (dangling ends) are not part of the score.
 * Outputs are HOST in all three forms:
 *   held_out[n_seq * P] (uint8, required): 0 = the segment has no match (exactly where the mm call's best_out is
 *     255); 1 = it has matches, none of them stable; 2 = at least one stable match, in either direction.
 *   t_best_out[n_seq * P] (double, optional): the greatest t_match over the segment's matches, the exact double;
 *     0.0 where held_out is 0.
 *   primer_segments_out[n_fwd + n_rev] (uint32, optional): segments with at least one match of the primer -- the mm
 *     call's array.
 *   primer_held_out[n_fwd + n_rev] (uint32, optional): segments with at least one STABLE match of the primer
 *     (segments, not positions; duplicate primers count independently).
 *   matches / capacity / count_out (optional; matches == NULL: no list): one msspe_scored_match per match, stable or
 *     not, dg and t raw, sorted by (primer, segment, offset).  The capacity contract is msspe_background_sites': when
 *     there are more matches than `capacity` the call returns MSSPE_ERR_CAPACITY, every other output and *count_out
 *     (the number of matches) are valid, and the first `capacity` records to arrive are kept, sorted.
 * Memory is bounded and nothing is dropped, as in msspe_background_thal*: the matches pass through the same work list
 * of 2^site_list_cap_log2 entries in slabs of whole segment groups (a group: the S <= 64 segments one block of the
 * comparison takes, 53 at window 50, k 13) against a range of primers.  A slab whose matches overrun the list -- the
 * listing kernel's counter runs past the capacity, nothing is written behind it -- is split by groups, then by
 * primers, and listed again; no output ever comes from a truncated list.  If one group against one primer still
 * overruns (more than 2^site_list_cap_log2 window positions in one group: at the minimum of 2^12 a window of more
 * than 4096 positions), the call returns MSSPE_ERR_CAPACITY and msspe_last_error names the option and both figures.
 * Routing is msspe_background_thal*'s over the explicit pair list; force_generic, wave_kernel, list_cap_log2 and
 * site_list_cap_log2 apply as there.  msspe_get_info "coverage_thal_*" describes the last call.  The call leaves the
 * context fit for any other call.
 * Errors: those of msspe_segment_coverage_mm*; MSSPE_ERR_K for k outside 2..31 (thal needs two bases); MSSPE_ERR_ARG
 * for a NULL chem or held_out, a mode outside {1, 2}, count_out NULL with a list, or a window of more than
 * 2^26 positions (W - k >= 2^26); MSSPE_ERR_TABLES as every dimer call.  No segments or no primers: MSSPE_OK, outputs zeroed, count 0. */
typedef struct {
    uint32_t primer;      /* 0 .. n_fwd + n_rev - 1, forward primers first */
    uint32_t segment;     /* r * P + j */
    uint32_t offset;      /* p, 0 .. W - k */
    uint16_t mismatches;  /* 0 .. max_mismatches */
    uint16_t stable;      /* 1 iff max(0, t) > msspe_t_cut(tm_threshold) */
    double dg, t;         /* raw */
} msspe_scored_match;
int msspe_segment_coverage_thal(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const uint64_t *fwd_words,
                                int n_fwd, const uint64_t *rev_words, int n_rev, const msspe_chem *chem, int mode,
                                float tm_threshold, uint8_t *held_out, double *t_best_out,
                                uint32_t *primer_segments_out, uint32_t *primer_held_out, msspe_scored_match *matches,
                                uint64_t capacity, uint64_t *count_out);
int msspe_segment_coverage_thal_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const uint64_t *fwd_words,
                                    int n_fwd, const uint64_t *rev_words, int n_rev, const msspe_chem *chem, int mode,
                                    float tm_threshold, uint8_t *held_out, double *t_best_out,
                                    uint32_t *primer_segments_out, uint32_t *primer_held_out,
                                    msspe_scored_match *matches, uint64_t capacity, uint64_t *count_out);
int msspe_segment_coverage_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                           const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                           const msspe_chem *chem, int mode, float tm_threshold, uint8_t *held_out,
                                           double *t_best_out, uint32_t *primer_segments_out,
                                           uint32_t *primer_held_out, msspe_scored_match *matches, uint64_t capacity,
                                           uint64_t *count_out);

/* ---- a panel thinned on the segments it holds at a temperature (engine extension, no reference counterpart) ----
 * msspe_panel_thin* keeps what the string rule's coverage needs; msspe_segment_coverage_thal* showed that a match
 * within M mismatches may score anywhere from 0 C to well above the reaction temperature, so a panel thinned on the
 * string rule may hold fewer segments afterwards than it did before.  These calls run the same greedy loop over the
 * HELD incidence.  The inputs are msspe_panel_thin*'s, plus chem, mode (1 ANY, 2 END1) and tm_threshold as in
 * msspe_segment_coverage_thal*; max_mismatches and exact_3p are the prefilter that says what a match is.
 *   H[p][s] = 1 when primer p has at least one STABLE match in segment s under exactly msspe_segment_coverage_thal*'s
 *     rule: that rule fixes the match, the template oligo, t_match = max(0, t) and "stable iff
 *     t_match > msspe_t_cut(tm_threshold)".  p, n and s as in msspe_panel_thin*.  A row sum of H is that call's
 *     primer_held_out[p]; a threshold <= 0 makes H the incidence I of msspe_panel_thin*.
 *   The greedy loop is msspe_panel_thin*'s, unchanged, over H instead of I: forced rows cover first and are never
 *     picked, a round picks the unforced, unpicked p of greatest gain, ties to the LOWEST index, until that gain is
 *     below thin->min_gain; keep_out, order_out, gain_out, *n_picked_out, covered_out, *covered_all_out (|OR of all
 *     H[p]|) and *covered_kept_out as there.
 * GUARANTEE: at min_gain 1 covered_out marks exactly the segments where the whole set's msspe_segment_coverage_thal*
 * held_out == 2, and the two counts are equal.  Stability is a property of (primer, template) alone, so
 * msspe_segment_coverage_thal* on the kept primers gives held_out == 2 on exactly the same segments: thinning loses no
 * held segment.  What it does NOT preserve: t_best per segment (a segment held at 45 C before may be held at 31 C
 * afterwards), and the segments that only had unstable matches (held_out == 1 may become 0).
 * Memory and routing: the matches pass through the work list of msspe_segment_coverage_thal* in slabs, with its
 * split-and-relist rule for a slab that overruns; the matrix is msspe_panel_thin*'s, under the same
 * "panel_thin_matrix_max_mb".  msspe_set_option "thin_thal_unique" ("0" / "1", default "1"): a slab's matches are
 * sorted by (primer, template word) and each distinct pair is scored once -- an alignment of related genomes repeats
 * its templates row after row; with "0" every match is scored, as msspe_segment_coverage_thal* does.  H, and so every
 * output, is the same either way.  force_generic, wave_kernel, list_cap_log2 and site_list_cap_log2 apply to the
 * scoring as there.  The call shares the context's work list and the thinning's buffers, leaves the context fit for any
 * other call, and allocates nothing once its buffers have grown to a call's size.
 * Errors: those of msspe_panel_thin* and of msspe_segment_coverage_thal*: MSSPE_ERR_K for k outside 2..31;
 * MSSPE_ERR_ARG for a mode outside {1, 2}, a NULL chem, thin or output array, min_gain < 1, or a window of more than
 * 2^26 positions; MSSPE_ERR_TABLES as every dimer call; MSSPE_ERR_CAPACITY when the matrix needs more than
 * panel_thin_matrix_max_mb, or when one segment group against one primer overruns the work list (msspe_last_error
 * names "site_list_cap_log2" and both figures).  n == 0 or no segments: as msspe_panel_thin*.
 * msspe_get_info, the last call: "panel_thin_thal_matches" (matches listed), "panel_thin_thal_unique_pairs" (pairs
 * scored: per slab the distinct ones, or with thin_thal_unique 0 the matches), "panel_thin_thal_slabs" /
 * "panel_thin_thal_redone" (slabs scored / listed again in parts), "panel_thin_thal_list_us" /
 * "panel_thin_thal_unique_us" / "panel_thin_thal_score_us" / "panel_thin_thal_fold_us" / "panel_thin_thal_rounds_us"
 * (device time of the listing, the templates with the sort and run search, the scoring, the fold, the rounds);
 * "panel_thin_rounds", "panel_thin_groups" and "panel_thin_gain0_us" describe this call too;
 * "thin_thal_unique" is the option's value. */
int msspe_panel_thin_thal(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                          const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const msspe_chem *chem, int mode,
                          float tm_threshold, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                          int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                          int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                          long long *covered_kept_out);
int msspe_panel_thin_thal_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                              const msspe_chem *chem, int mode, float tm_threshold, const uint64_t *fwd_words,
                              int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                              uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                              uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out);
int msspe_panel_thin_thal_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                     const msspe_thin_opt *thin, const msspe_chem *chem, int mode, float tm_threshold,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                     int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                                     long long *covered_kept_out);

/* ---- a panel thinned to a coverage depth: R primers on every segment (engine extension, no reference counterpart;
 * DESIGN.md 4.15) ----
 * msspe_panel_thin* and msspe_panel_thin_thal* leave many segments on exactly one primer; one mutation under its 3' end
 * loses the segment.  These calls keep at least R primers on every segment wherever the panel has that many.  The
 * inputs are the sibling's, with msspe_thin_depth_opt {min_gain >= 1, depth R in 1..255} in place of msspe_thin_opt.
 *   Incidence.  I[p][s] of msspe_panel_thin*; the thal forms use the held incidence H of msspe_panel_thin_thal*.
 *   Shadows.  Among primers with the same (direction, word) one is the representative: the forced one of lowest index
 *     if any is forced, otherwise the lowest index.  All the others are shadows: a shadow counts in nothing, is never
 *     picked, and its keep_out is its forced flag.  (At depth 2 a word listed twice would otherwise pass for two
 *     primers.)  A forward word equal to a reverse word is no duplicate: the two look in different windows.
 *   Counters.  depth_all[s] = representatives with I[p][s]; need[s] = min(R, depth_all[s]); cnt[s] starts as
 *     min(need[s], forced representatives with I[p][s]); s is open while cnt[s] < need[s].
 *   Rounds.  gain(p) = open segments with I[p][s], over the representatives neither forced nor picked; the greatest
 *     gain is picked, ties to the lowest index; below min_gain the loop ends and nothing is picked in that round;
 *     otherwise p joins the order with its gain and cnt[s] += 1 on every open s with I[p][s].
 *   Outputs.  keep_out[n], order_out, gain_out, *n_picked_out as msspe_panel_thin*.  depth_all_out / depth_kept_out
 *     (optional host arrays, n_seq * P bytes, s = r * P + j): representatives per segment among all primers and among
 *     the kept ones, saturating at 255; depth_kept is the true column sum, not cnt.  counts_out[4] (optional):
 *     segments with depth_all >= 1, depth_kept >= 1, depth_all >= R, depth_kept >= R.
 *   Guarantee at min_gain 1: depth_kept[s] >= min(R, depth_all[s]) for every s (an open segment at the end would give
 *     an unpicked live representative a gain of 1), so counts[1] == counts[0] and counts[3] == counts[2].
 *   At depth 1 keep_out, order_out, gain_out, *n_picked_out and "panel_thin_rounds" are those of the sibling on the same
 *     inputs, duplicates and forced flags included.  As in the siblings, the best mismatch count per segment (thal
 *     forms: t_best) is NOT preserved.
 * Errors: those of the sibling, plus MSSPE_ERR_ARG for a depth outside 1..255.  n == 0 or no segments: as the sibling,
 * with the counts zeroed.  The calls share "panel_thin_matrix_max_mb" and every buffer of the thinning; once the buffers
 * have grown to a call's size, the calls allocate nothing.  msspe_get_info: the "panel_thin_*" and "panel_thin_thal_*"
 * keys describe these calls too; "panel_thin_depth_shadows" is the last depth call's number of shadows,
 * "panel_thin_depth_colsum_us" its device time in the three column-sum passes (all, forced, kept) and the needs. */
typedef struct { int min_gain; int depth; } msspe_thin_depth_opt;   /* min_gain >= 1, depth 1..255 */
int msspe_panel_thin_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                           const msspe_mismatch_opt *mm, const msspe_thin_depth_opt *thin, const uint64_t *fwd_words,
                           int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                           uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                           uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_thin_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                               const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                               const msspe_thin_depth_opt *thin, const uint64_t *fwd_words, int n_fwd,
                               const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                               uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                               uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_thin_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                      const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                      const msspe_thin_depth_opt *thin, const uint64_t *fwd_words, int n_fwd,
                                      const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                                      uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                      uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_thin_thal_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode, float tm_threshold,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                long long *counts_out);
int msspe_panel_thin_thal_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                    const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode,
                                    float tm_threshold, const uint64_t *fwd_words, int n_fwd,
                                    const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out,
                                    uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_thin_thal_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                           const msspe_thin_depth_opt *thin, const msspe_chem *chem, int mode,
                                           float tm_threshold, const uint64_t *fwd_words, int n_fwd,
                                           const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                           uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                           int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                           long long *counts_out);

/* ---- a conflict-free panel selected by coverage: set cover under conflicts (engine extension, no reference
 * counterpart) ----
 * msspe_conflict_cover* deletes primers by conflict degree and never looks at coverage: it deletes the only primer that
 * primes a segment as readily as one of five that prime the same segment, and msspe_panel_thin* cannot bring the
 * segment back.  These calls join the two steps: a greedy set cover in which a pick bars its conflict neighbours --
 * with more than one tube, from its own tube only.
 *   Inputs.  The inputs of msspe_panel_thin* are kept: alignment, msspe_kmer_opt, forward and reverse primer words,
 *     optional forced flags, min_gain >= 1.  The incidence rule is given as a msspe_seed_rule: mode 0 is the string
 *     rule I of msspe_panel_thin*; modes 1 and 2 are the held incidence H of msspe_panel_thin_thal*; a threshold <= 0
 *     gives mode 0's matrix.  New inputs: max_tubes = T, 1..64; drop_self_pairs; and a conflict bitmap B over the
 *     index p.  p runs over the forward primers in the caller's order, then the reverse primers, n = n_fwd + n_rev.  B
 *     is n x ceil(n/64) words in the layout msspe_cross_dimer_dev writes for the pool "forward words then reverse
 *     words".  Reverse words are in primer orientation, as the CSV writes them.
 *   Graph.  This is the cover's graph.  S = B | B^T, padding bits ignored.  With drop_self_pairs the diagonal and the
 *     reverse-complement partners are cleared first.  The words must be distinct across both lists, exactly as
 *     msspe_conflict_cover* checks; duplicate words and bits above 2 k are MSSPE_ERR_ARG.  p is SELF-CONFLICTING when
 *     S[p][p] is still set.
 *   State.  covered starts as the OR of the forced rows.  mask[p] is a 64-bit set of tubes barred to p.  Every
 *     neighbour of a forced primer starts with all T bits set, because the panel is in every tube.  Everyone else
 *     starts at 0.  p is LIVE when it is not forced, not picked, not self-conflicting, and mask[p] lacks at least one
 *     of the low T bits.
 *   Rounds.  Each round computes gain(p) = |row(p) & ~covered| over the live p.
 *     1. The round takes the greatest gain.  Ties go to the LOWEST index.
 *     2. If that gain is below min_gain, or nobody is live, the loop ends.
 *     3. Otherwise p is appended to the order with its gain, and tube(p) = the lowest tube not in mask[p].
 *     4. covered |= row(p).
 *     5. mask[u] |= 1 << tube(p) for every u != p with S[p][u] set.
 *   Outputs.  keep_out[n]: forced or picked.  order_out, gain_out (the caller sizes both to n), *n_picked_out.
 *     tube_out[n]: the tube of a pick; MSSPE_TUBE_NONE for everyone else, forced primers included.  barred_out[n]
 *     (optional): 1 for a primer not kept that is self-conflicting or whose low T mask bits are all set at the end.
 *     covered_out (optional, n_seq * P bytes), *covered_all_out (optional: the whole set's coverage, conflicts
 *     ignored), *covered_kept_out (optional).  *n_tubes_used_out (optional).
 * GUARANTEES.  No two picks of one tube are neighbours in S, and no pick is a neighbour of a forced primer.  The tubes
 * in use are 0 .. used - 1, without gaps.  With an all-zero bitmap and any T, the order, gains, keep, covered and both
 * counts are msspe_panel_thin*'s (mode 0) or msspe_panel_thin_thal*'s (modes 1 and 2), and every pick is in tube 0.  On
 * a complete graph without self loops, the picks are the first min(T, picks) picks of the plain thinning, in tubes 0,
 * 1, 2, ....  What the rule does NOT promise: that covered_kept == covered_all (conflicts may cost segments), or a
 * maximum.  It is greedy.
 * Limits: n <= 262,144 (MSSPE_ERR_ARG above it), "panel_thin_matrix_max_mb" (MSSPE_ERR_CAPACITY, never a partial run),
 * k in 2..31 (MSSPE_ERR_K).  Errors: those of msspe_panel_thin* / msspe_panel_thin_thal* and of msspe_conflict_tubes*;
 * max_tubes outside 1..64, a NULL rule, sel, bitmap or output array (keep_out, order_out, gain_out, n_picked_out,
 * tube_out), a mode outside 0..2 and a NULL rule->chem in modes 1 and 2 are MSSPE_ERR_ARG.  n == 0 or no segments:
 * MSSPE_OK with nothing picked and keep_out = the forced flags.
 * msspe_get_info, the last call: "panel_select_rounds" (the picks and the round that stopped), "panel_select_tubes",
 * "panel_select_barred", "panel_select_prepare_us" (ranks, duplicate check and S), "panel_select_incidence_us",
 * "panel_select_first_us" (forced rows, first barring, first gains) and "panel_select_rounds_us".
 *
 * The _dev forms read the alignment from the device (bytes / packed rows, as msspe_panel_thin_dev / _packed_dev) and
 * d_bitmap (device, read only); every other argument is on the host.  They share the cover's S, the thinning's matrix
 * and, in modes 1 and 2, the work list with the other calls of the context, and allocate nothing once their buffers
 * have grown to a call's size.  msspe_panel_select takes the alignment on the host and screens the pool itself
 * (msspe_cross_dimer_dev, bitmap only, decisions path, as msspe_conflict_tubes does) with chem and dg_threshold.
 * msspe_panel_select_bitmap takes the alignment and the n x ceil(n/64) bitmap from the host. */
typedef struct {
    int min_gain;          /* >= 1: a pick must cover at least this many segments nothing kept covers yet */
    int max_tubes;         /* 1..64 */
    int drop_self_pairs;   /* as msspe_conflict_cover* */
} msspe_select_opt;

int msspe_panel_select_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                           const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words,
                           int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                           const uint64_t *d_bitmap, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                           int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                           long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out);
int msspe_panel_select_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  const uint8_t *forced, const uint64_t *d_bitmap, uint8_t *keep_out,
                                  uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                                  uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                                  long long *covered_kept_out, int *n_tubes_used_out);
int msspe_panel_select(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                       const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                       const uint64_t *rev_words, int n_rev, const uint8_t *forced, const msspe_chem *chem,
                       float dg_threshold, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                       int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                       long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out);
int msspe_panel_select_bitmap(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              const uint8_t *forced, const uint64_t *bitmap, uint8_t *keep_out, uint32_t *order_out,
                              uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                              uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
                              int *n_tubes_used_out);
/* msspe_panel_select with the conflict rule in place of dg_threshold: the pool is screened with
 * msspe_conflict_graph_dev (bitmap only); the rest is msspe_panel_select_dev.  A NULL conflict_rule or both flags
 * zero: MSSPE_ERR_ARG. */
int msspe_panel_select_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                            const msspe_seed_rule *rule, const msspe_select_opt *sel, const uint64_t *fwd_words,
                            int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                            const msspe_chem *chem, const msspe_conflict_rule *conflict_rule, uint8_t *keep_out,
                            uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
                            uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                            long long *covered_kept_out, int *n_tubes_used_out);

/* ---- a conflict-free panel selected to a coverage depth, layer by layer (engine extension, no reference
 * counterpart) ----
 * msspe_panel_select* stops once every reachable segment has ONE primer, and msspe_panel_thin_depth* knows no
 * conflicts.  These calls select a conflict-free, tube-assigned panel in which a segment keeps up to R primers.  The
 * depth thinning's rule ("open while cnt < min(R, depth_all)") cannot simply take the barring on: a pick made for its
 * second-primer gains bars the only primer of other segments, and breadth is lost.  The rule here runs in LAYERS, so
 * that asking for depth never costs breadth: layer 1 is exactly msspe_panel_select*, layer r then adds primers for the
 * segments that still have fewer than r.
 *   Inputs.  Everything msspe_panel_select* takes, with msspe_select_depth_opt {min_gain >= 1, max_tubes 1..64,
 *     drop_self_pairs, depth = R in 1..255} in place of msspe_select_opt.  The words must be distinct across both
 *     lists, as there; so there are no shadows (msspe_panel_thin_depth*).
 *   Graph, SELF-CONFLICTING, mask, LIVE and the choice of the tube are msspe_panel_select*'s.
 *   State, carried through the whole run.  depth_all[s] = the number of the n primers with I[p][s]; conflicts are
 *     ignored, as for covered_all.  cnt[s] = the number of kept (forced or picked) primers with I[p][s]: the true count,
 *     which starts from the forced rows.  mask starts as in msspe_panel_select*.  D = max_s depth_all[s].
 *   Layers r = 1 .. L run in order, L = min(R, max(1, D)).  In layer r, segment s is OPEN while
 *     cnt[s] < min(r, depth_all[s]).  A round of layer r:
 *     1. gain(p) = |{s : I[p][s], s open}| over the live p.
 *     2. The greatest gain wins.  Ties go to the LOWEST index.
 *     3. If nobody is live, or the greatest gain is below min_gain, the round picks nothing and the layer ends.  That
 *        stopping round counts as a round.
 *     4. Otherwise p joins the order with its gain and its layer.
 *     5. tube(p) = the lowest tube not in mask[p].
 *     6. cnt[s] += 1 on EVERY s with I[p][s], open or not, saturating at 255.
 *     7. mask[u] |= 1 << tube(p) for every u != p with S[p][u] set.
 *     Barring, picks and cnt carry over from layer to layer.  Rounds reported = picks + L.
 *   Outputs.  keep_out, order_out, gain_out, *n_picked_out, tube_out, barred_out (optional) and *n_tubes_used_out
 *     (optional) as msspe_panel_select*.  pick_layer_out (optional, uint8 per position of the order; the caller sizes it
 *     to n): the layer of the pick.  depth_all_out and depth_kept_out (optional, n_seq * P bytes, saturating at 255;
 *     depth_kept = the final cnt).  counts_out[4] (optional): segments with depth_all >= 1, depth_kept >= 1,
 *     depth_all >= R, depth_kept >= R.
 * GUARANTEES.
 *   R = 1 is msspe_panel_select*: order, gains, keep, tube, barred, tubes used and "panel_select_rounds" are equal,
 *     and counts[0..1] = (covered_all, covered_kept).
 *   Prefix.  The run at depth R - 1 is a prefix of the run at depth R: same order, gains, layers and tubes on the
 *     prefix.  So counts[1] never falls as R grows; at min_gain 1 it does not change at all, because after layer 1 no
 *     live primer has an uncovered segment.
 *   Independence.  msspe_panel_select*'s guarantee is unchanged: no two picks of one tube are neighbours in S, no pick
 *     is a neighbour of a forced primer, the tubes in use are 0 .. used - 1.
 *   With an all-zero bitmap at min_gain 1: depth_kept[s] >= min(R, depth_all[s]) for every s.
 *   Gains.  The sum of the gains of the picks of layer r = the sum over s of min(cnt_end[s], m[s]) - min(cnt_start[s],
 *     m[s]), with m[s] = min(r, depth_all[s]) and cnt at the layer's start and end: every hit a segment takes while open
 *     counts once.
 * What the rule does NOT promise: equality with the thinning -- with a zero bitmap the picks are in general not
 * msspe_panel_thin_depth*'s, because that rule is not layered (the kept count may coincide); any depth under conflicts;
 * or a maximum.  It is greedy.
 * Limits and errors: those of msspe_panel_select*; depth outside 1..255 is MSSPE_ERR_ARG.  n == 0 or no segments:
 * MSSPE_OK with nothing picked, keep_out = the forced flags and counts 0.
 * msspe_get_info, the last call: the "panel_select_*" keys, with "panel_select_first_us" now the first barring, the
 * column sums and layer 1's init and first gains, and "panel_select_rounds_us" everything after; and
 * "panel_select_depth_layers" (L) and "panel_select_depth_layer_us" (the column sums and every layer's init and first
 * gains).
 * The five forms mirror msspe_panel_select_dev, _packed_dev, msspe_panel_select (screens the pool itself at
 * dg_threshold), _bitmap and _rule; the incidence modes 0 / 1 / 2 of msspe_seed_rule are unchanged. */
typedef struct {
    int min_gain;          /* >= 1 */
    int max_tubes;         /* 1..64 */
    int drop_self_pairs;   /* as msspe_conflict_cover* */
    int depth;             /* R, 1..255 */
} msspe_select_depth_opt;

int msspe_panel_select_depth_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                 const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                 const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint64_t *d_bitmap,
                                 uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                 uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out,
                                 uint8_t *pick_layer_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                 long long *counts_out);
int msspe_panel_select_depth_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                        const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                        const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                        const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                        const uint64_t *d_bitmap, uint8_t *keep_out, uint32_t *order_out,
                                        uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                                        int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                                        uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_select_depth(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                             const msspe_seed_rule *rule, const msspe_select_depth_opt *sel, const uint64_t *fwd_words,
                             int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                             const msspe_chem *chem, float dg_threshold, uint8_t *keep_out, uint32_t *order_out,
                             uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                             int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                             uint8_t *depth_kept_out, long long *counts_out);
int msspe_panel_select_depth_bitmap(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                    const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                    const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint64_t *bitmap,
                                    uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out,
                                    uint8_t *pick_layer_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                                    long long *counts_out);
int msspe_panel_select_depth_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                  const msspe_select_depth_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                  const uint64_t *rev_words, int n_rev, const uint8_t *forced, const msspe_chem *chem,
                                  const msspe_conflict_rule *conflict_rule, uint8_t *keep_out, uint32_t *order_out,
                                  uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out,
                                  int *n_tubes_used_out, uint8_t *pick_layer_out, uint8_t *depth_all_out,
                                  uint8_t *depth_kept_out, long long *counts_out);

/* ---- weighted coverage: thinning and selection on a weight per segment (engine extension, no reference
 * counterpart) ----
 * msspe_panel_thin* and msspe_panel_select* count every segment as 1, so 9,000 near-identical genomes of one lineage
 * outvote 40 of a rare clade.  These calls take a weight per segment and are otherwise their unweighted siblings, at
 * depth 1: the arguments, limits, errors and msspe_get_info keys ("panel_thin_*", "panel_select_*") are the sibling's.
 *   weights (host, n_seq * P entries, uint32): weights[s], s = r * P + j, in the order of best_out / covered_out.
 *   gain(p) = the SUM of weights[s] over the segments s with I[p][s] set and covered[s] clear.  The pick is the greatest
 *     gain, ties to the lowest index; the loop ends when that gain is below min_gain, which is in WEIGHT UNITS here (and
 *     >= 1).  gain_out holds weights.  Covering, forcing, barring, tubes and every other output are unchanged.
 *   A segment of weight 0 never contributes to a gain, so no primer is spent on it; it still gets its covered bit when a
 *     pick happens to cover it: covered_out, *covered_all_out and *covered_kept_out stay the real coverage, in segments.
 *   *weight_all_out / *weight_kept_out (optional): the weight of the segments that the whole set covers and that the
 *     kept set covers.
 *   The weights' total over all segments must be <= 2^32 - 1, so that every gain fits the high half of the pick key
 *     gain << 32 | ~p: above it the call returns MSSPE_ERR_ARG with both figures in msspe_last_error.  weights == NULL is
 *     MSSPE_ERR_ARG: the unweighted call exists for that case.
 * GUARANTEES.  (1) With all weights 1 every output equals the unweighted call's: keep, order, gains, covered, both
 * counts, tubes, barred (and the two weights equal the two counts).  (2) For the thinning at min_gain 1,
 * *weight_kept_out == *weight_all_out: no segment of positive weight that the whole set covers is lost.  The selection
 * does not promise this, as it does not promise it unweighted: conflicts may cost segments -- the weights decide which.
 * The thinning forms use the string rule of msspe_panel_thin*.  The selection forms take the msspe_seed_rule modes 0..2
 * as msspe_panel_select* does; the _rule form screens the pool itself under a msspe_conflict_rule (use_end = 0 gives the
 * dG-only screen of msspe_panel_select). */
int msspe_panel_thin_weighted(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                              const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words,
                              int n_fwd, const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                              const uint32_t *weights, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                              int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                              long long *covered_kept_out, uint64_t *weight_all_out, uint64_t *weight_kept_out);
int msspe_panel_thin_weighted_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                  const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                  const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                  const uint8_t *forced, const uint32_t *weights, uint8_t *keep_out,
                                  uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                                  long long *covered_all_out, long long *covered_kept_out, uint64_t *weight_all_out,
                                  uint64_t *weight_kept_out);
int msspe_panel_thin_weighted_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                         const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm,
                                         const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                                         const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                         const uint32_t *weights, uint8_t *keep_out, uint32_t *order_out,
                                         uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                                         long long *covered_all_out, long long *covered_kept_out,
                                         uint64_t *weight_all_out, uint64_t *weight_kept_out);
int msspe_panel_select_weighted_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                    const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                    const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                    const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights,
                                    uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                    uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                    long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                    uint64_t *weight_all_out, uint64_t *weight_kept_out);
int msspe_panel_select_weighted_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                           const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                           const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                           const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                           const uint64_t *d_bitmap, const uint32_t *weights, uint8_t *keep_out,
                                           uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                           uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                           long long *covered_all_out, long long *covered_kept_out,
                                           int *n_tubes_used_out, uint64_t *weight_all_out, uint64_t *weight_kept_out);
int msspe_panel_select_weighted_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, const msspe_chem *chem,
                                     const msspe_conflict_rule *conflict_rule, const uint32_t *weights,
                                     uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                     uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                     long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                     uint64_t *weight_all_out, uint64_t *weight_kept_out);

/* ---- primer costs: thinning and selection by coverage per cost (engine extension, no reference counterpart;
 * DESIGN.md 4.18) ----
 * The calls above treat every primer as equally good: a pick is decided by gain alone.  These calls take a cost per
 * primer and are otherwise their siblings at depth 1 -- msspe_panel_thin_weighted* / msspe_panel_select_weighted* with
 * weights, msspe_panel_thin* / msspe_panel_select* without: the arguments, limits, errors and msspe_get_info keys
 * ("panel_thin_*", "panel_select_*") are the sibling's.  Weights say which segments matter, costs which primers to
 * prefer: together the weighted set cover.
 *   costs (host, n_fwd + n_rev entries, uint32, each >= 1): costs[p] in the order of keep_out, forward list then reverse.
 *   weights (host, optional): as in the weighted calls.  NULL means every segment counts 1; *weight_all_out /
 *     *weight_kept_out, where given, then receive the two covered counts.
 *   gain(p) is unchanged: the sum of weights[s] (or the number) of the uncovered segments of row p.  A round considers
 *     the live primers whose gain is at least min_gain and picks the greatest gain(p) / cost(p).  The comparison is exact:
 *     p beats q when gain(p) * cost(q) > gain(q) * cost(p) in 64-bit unsigned arithmetic (both factors are below 2^32);
 *     on equal products the greater gain wins, then the lowest index.  A primer whose gain is below min_gain is no
 *     candidate, whatever its ratio.  When no live primer qualifies the loop ends; that round counts.  gain_out holds
 *     gains, not ratios.  Covering, forcing, barring, tubes and every other output are the sibling's.
 *   *cost_all_out / *cost_kept_out (optional): the sum of costs over all primers and over keep_out == 1, forced primers
 *     included.
 *   costs == NULL or a cost of 0 is MSSPE_ERR_ARG; msspe_last_error names the first offending index.  The weights' total
 *     is bounded by 2^32 - 1 as in the weighted calls.
 * GUARANTEES.  (1) With all costs equal to any constant c >= 1 every output equals the sibling's: keep, order, gains,
 * covered, both counts, both weights, tubes, barred and the rounds run.  (2) The thinning at min_gain 1 still loses
 * nothing: *covered_kept_out == *covered_all_out, and with weights *weight_kept_out == *weight_all_out.  The selection
 * promises neither, as before.  (3) The kept set of the selection is independent under the graph, tube by tube, as in
 * msspe_panel_select*.  Depth 1 only. */
int msspe_panel_thin_cost(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len, const msspe_kmer_opt *opt,
                          const msspe_mismatch_opt *mm, const msspe_thin_opt *thin, const uint64_t *fwd_words, int n_fwd,
                          const uint64_t *rev_words, int n_rev, const uint8_t *forced, const uint32_t *weights,
                          const uint32_t *costs, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                          int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                          long long *covered_kept_out, uint64_t *weight_all_out, uint64_t *weight_kept_out,
                          uint64_t *cost_all_out, uint64_t *cost_kept_out);
int msspe_panel_thin_cost_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                              const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                              const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                              const uint8_t *forced, const uint32_t *weights, const uint32_t *costs, uint8_t *keep_out,
                              uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out,
                              long long *covered_all_out, long long *covered_kept_out, uint64_t *weight_all_out,
                              uint64_t *weight_kept_out, uint64_t *cost_all_out, uint64_t *cost_kept_out);
int msspe_panel_thin_cost_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                     const msspe_kmer_opt *opt, const msspe_mismatch_opt *mm, const msspe_thin_opt *thin,
                                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                     const uint8_t *forced, const uint32_t *weights, const uint32_t *costs,
                                     uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                     uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
                                     uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                     uint64_t *cost_kept_out);
int msspe_panel_select_cost_dev(msspe_ctx *ctx, const uint8_t *d_seqs, int n_seq, size_t seq_len,
                                const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                const uint8_t *forced, const uint64_t *d_bitmap, const uint32_t *weights,
                                const uint32_t *costs, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                uint64_t *cost_kept_out);
int msspe_panel_select_cost_packed_dev(msspe_ctx *ctx, const uint64_t *d_packed, int n_seq, size_t seq_len,
                                       const msspe_kmer_opt *opt, const msspe_seed_rule *rule,
                                       const msspe_select_opt *sel, const uint64_t *fwd_words, int n_fwd,
                                       const uint64_t *rev_words, int n_rev, const uint8_t *forced,
                                       const uint64_t *d_bitmap, const uint32_t *weights, const uint32_t *costs,
                                       uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                                       uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                       long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                       uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                       uint64_t *cost_kept_out);
int msspe_panel_select_cost_rule(msspe_ctx *ctx, const uint8_t *seqs, int n_seq, size_t seq_len,
                                 const msspe_kmer_opt *opt, const msspe_seed_rule *rule, const msspe_select_opt *sel,
                                 const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                                 const uint8_t *forced, const msspe_chem *chem,
                                 const msspe_conflict_rule *conflict_rule, const uint32_t *weights,
                                 const uint32_t *costs, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                                 int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out,
                                 long long *covered_all_out, long long *covered_kept_out, int *n_tubes_used_out,
                                 uint64_t *weight_all_out, uint64_t *weight_kept_out, uint64_t *cost_all_out,
                                 uint64_t *cost_kept_out);

/* ---- several devices of one node ----------------------------------------------------------
 *
 * One process, one context and one host thread per device.  What shards is the reference's N^2 pair loop
 * (od-msspe/src/delta_g.rs:61-81, called at main.rs:739-752: every ordered pair is independent) and the per-oligo
 * statistics (od-msspe/src/primer.rs:143-166); stage A's greedy loop is sequential and runs on member 0's context
 * (msspe_group_member(g, 0) with the msspe_kmer_candidates* calls).
 *
 * A screen: every member uploads the slice of the pool it "produced" (contiguous n / N candidates), ONE all-gather
 * assembles the packed pool on every device, every member screens its rows against all columns, ONE all-reduce
 * merges the per-primer conflict counts; bitmap rows and edge lists stay with their member until the host call
 * collects them.  Rows are dealt out in groups of 256, round robin (row r belongs to member (r / 256) mod N), so
 * that every member gets a sample of the whole pool whatever its order (msspe_group_rows lists a member's rows).
 * Results are identical to the single-context calls (tests/test_gpu_group.py: members that share one card -- the
 * device-copy transport -- and RCCL as a group of one rank).  NOT YET VERIFIED ON HARDWARE: two or more DISTINCT
 * devices (grouped ncclAllGather / ncclAllReduce on N communicators from one thread, peer access, cross-device copies);
 * no multi-GPU node has been reachable from the build, the two-device test skips on one card.
 *
 * transport: "auto" (NULL) | "rccl" | "device-copy".  "rccl": RCCL over xGMI, librccl.so loaded when the group is
 * made, needs distinct devices.  "device-copy": device-to-device copies and a summing kernel -- for members that
 * share a card (a device may be listed more than once: how the tests rehearse N members on one GPU) and where
 * RCCL cannot be loaded.  auto = rccl for two or more distinct devices if it loads, else device-copy.
 */
typedef struct msspe_group msspe_group;
int msspe_group_create(const int *devices, int n_devices, const char *params_path, const char *transport,
                       msspe_group **out);
void msspe_group_destroy(msspe_group *g);
const char *msspe_group_last_error(const msspe_group *g);
int msspe_group_size(const msspe_group *g);
const char *msspe_group_transport(const msspe_group *g);          /* "single" | "rccl" | "device-copy" */
/* "" unless transport "auto" wanted RCCL and runs the copies instead: then why (librccl.so not loadable,
 * ncclCommInitAll's error, or the failure of the first grouped collective, which msspe_group_create runs with a
 * known answer before any screen depends on the fabric) */
const char *msspe_group_transport_reason(const msspe_group *g);
/* Host only, no device: 1 if RCCL (library: NULL = the names msspe_group_create tries) can be loaded with every
 * collective entry point the group uses, else 0 and the reason in why[0 .. why_capacity) */
int msspe_group_rccl_available(const char *library, char *why, int why_capacity);
msspe_ctx *msspe_group_member(msspe_group *g, int member);        /* owned by the group */
int msspe_group_set_option(msspe_group *g, const char *key, const char *value);   /* msspe_set_option on every member */
/* pool rows member `member` of a group of n_members screens in a pool of n (ascending).  Host only, no device.
 * *n_rows_out is set even when capacity is 0 (sizing call); a capacity that is too small: MSSPE_ERR_CAPACITY */
int msspe_group_rows(int n, int n_members, int member, uint32_t *rows_out, int capacity, int *n_rows_out);
/* msspe_cross_dimer over the group (host buffers; row_conflicts[n] merged, bitmap[n * ceil(n/64)] optional) */
int msspe_cross_dimer_group(msspe_group *g, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                            float dg_threshold, uint32_t *row_conflicts, uint64_t *bitmap);
/* msspe_cross_dimer_edges over the group: same order, same rounding, same capacity contract */
int msspe_cross_dimer_edges_group(msspe_group *g, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                                  float dg_threshold, msspe_edge *edges, uint64_t capacity, uint64_t *count_out);
/* msspe_oligo_stats over the group (contiguous slices of the oligos, one per member) */
int msspe_oligo_stats_group(msspe_group *g, const char *pool_ascii, int n, int k, const msspe_chem *chem,
                            double *tm, double *gc, double *self_any, double *self_end, double *hairpin);

/* ---- text rounding at the reference's process boundary ----------- */

float msspe_round_g_f32(double x);                  /* "%g"   -> f32 (od-msspe/src/delta_g.rs:33-35) */
float msspe_round_fixed_f32(double x, int decimals);/* "%.Nf" -> f32 (od-msspe/src/primer.rs:94-106) */
/* Largest double X such that msspe_round_g_f32(x) < threshold  <=>  x <= X (the decision cut the
 * kernels compare against; exact by construction, found by bisection over doubles). */
double msspe_g_cut(float threshold);
/* Largest double X such that msspe_round_fixed_f32(x, 2) < tm_threshold  <=>  x <= X: the END screen's cut (a pair
 * conflicts iff t_end > X); below 0 when tm_threshold <= 0, so that every pair conflicts. */
double msspe_t_cut(float tm_threshold);

#ifdef __cplusplus
}
#endif
#endif
