// od_msspe.hpp -- C++ host side above the C ABI, mirroring the reference's (Rust) interface for
// the hot path and the rows SURVEY.md 8f marks "next": same names, argument meaning and error
// behaviour as /root/reference/od-msspe/src/{main,primer,delta_g,config,constants}.rs.
// Everything thermodynamic or k-mer related is computed by libmsspe_hip.so (no CPU fallback);
// what stays on the host is what the north star leaves on the host: FASTA I/O, the outer
// pipeline, the (tiny, sequential) vertex cover, the report and the CSV.
#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/msspe_hip.h"

namespace od_msspe {

// constants.rs:1-26
constexpr int KMER_SIZE = 13, WINDOW_SIZE = 500, OVERLAP_SIZE = 250, MAX_ITERATIONS = 1000,
              SEARCH_WINDOWS_SIZE = 50;
constexpr float MV_CONC = 50.0f, DV_CONC = 3.0f, DNTP_CONC = 0.0f, DNA_CONC = 250.0f,
                ANNEALING_TEMP = 25.0f, PRIMER_MIN_TM = 30.0f, PRIMER_MAX_TM = 60.0f,
                PRIMER_MAX_SELF_ANY_TH = 47.0f, PRIMER_MAX_SELF_END_TH = 47.0f,
                PRIMER_MAX_HAIRPIN_TH = 24.0f, DELTA_G_THRESHOLD = -9000.0f;
constexpr uint8_t SEQ_DIR_FWD = 0, SEQ_DIR_REV = 1;

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct Panic : std::runtime_error {   // where the reference panics
    using std::runtime_error::runtime_error;
};

// config.rs:11-148 (clap Args; every option except -i/-o also reads an environment variable)
struct Args {
    std::string input, output;
    int kmer_size = KMER_SIZE, window_size = WINDOW_SIZE, overlap_size = OVERLAP_SIZE;
    int max_mismatch_segments = -1;   // Option<usize>: -1 = not given
    int max_iterations = MAX_ITERATIONS, search_windows_size = SEARCH_WINDOWS_SIZE;
    float mv_conc = MV_CONC, dv_conc = DV_CONC, dntp_conc = DNTP_CONC, dna_conc = DNA_CONC,
          annealing_temp = ANNEALING_TEMP, min_tm = PRIMER_MIN_TM, max_tm = PRIMER_MAX_TM,
          max_self_dimer_any_tm = PRIMER_MAX_SELF_ANY_TH, max_self_dimer_end_tm = PRIMER_MAX_SELF_END_TH,
          max_hairpin_tm = PRIMER_MAX_HAIRPIN_TH, delta_g_threshold = DELTA_G_THRESHOLD;
    std::string keep_all = "false", check_cross_dimers = "true", check_self_dimers = "true",
                check_hairpin = "true", disable_tm_stddev = "false", disable_min_max_tm = "false",
                do_align = "true";
    float tm_stddev = 2.0f;
    std::string ntthal = "ntthal", primer3 = "primer3_core";   // accepted for compatibility, unused
    // engine-only switches (not in the reference)
    int device = 0;
    std::string devices;           // "0,1,2,...": the N^2 pair loop and stage B run on a group of devices (msspe_group_*)
    std::string params_path;       // Primer3 config directory; empty = bundled tables
    std::string existing_primers;  // a panel to extend: CSV in this tool's output format (direction and primers read)
    // --exclude-primers FILE: words stage A must never pick (msspe_kmer_candidates_*sets*), read like a panel CSV
    // (direction and primers; further columns ignored, so the file of --rejected-out can be given).  --rejected-out
    // FILE: every candidate this run dropped, as direction,name,primers,round,reason (reason: stage_b, background,
    // panel_dimer or cover; --select-by-coverage: select_conflict or select_unneeded).  --repick-rounds N (0..16):
    // after the first pass, up to N more passes that keep what passed, ban what failed and let stage A fill the holes, each run like an --existing-primers run whose panel is
    // the user's plus everything kept so far.  One device, not with --tubes.  0 / empty: nothing changes.
    std::string exclude_primers, rejected_out;
    int repick_rounds = 0;
    std::string cover_on_device = "false";   // "true": the screen and the vertex cover as one device call (msspe_conflict_cover)
    // --tubes N (1..64): instead of the vertex cover, the primers are split into at most N reaction tubes in which no
    // two primers conflict (msspe_conflict_tubes); the primers that fit no tube are dropped, the CSV gains a 1-based
    // "tube" column and the report a block.  Not a better cover at N = 1.  0: nothing changes.
    int tubes = 0;
    // > 0: after the exact report, a second one counting a segment covered when a primer matches within this many
    // mismatches, its last coverage_3p_exact bases exact (msspe_segment_coverage_mm); 0: nothing changes
    int coverage_mismatches = 0;
    std::string coverage_3p_exact_text = "3";   // read (as an integer) only when coverage_mismatches > 0
    int coverage_3p_exact = 3;
    // --coverage-tm C: after the coverage report(s), the segments the final primers hold at C -- every match within
    // coverage_mismatches (its last coverage_3p_exact bases exact; both are read with this switch too) is scored with
    // thal against the strand the primer anneals to (msspe_segment_coverage_thal, --coverage-thal any | end1, the
    // cross-dimer screen's chemistry); a match is stable iff round_fixed_f32(max(0, t), 2) >= C.  One device.
    // Empty text: not given, nothing changes (and --coverage-thal is not read).
    std::string coverage_tm_text, coverage_thal;
    float coverage_tm = 0.0f;
    bool coverage_scored = false;
    // --max-cross-dimer-end-tm <C>: a pair of primers also conflicts when thal END1 of either order holds at C
    // (od-msspe's SELF_END rule applied to the pair); absent: the dG rule alone, every output as before
    std::string max_cross_dimer_end_tm_text;
    float max_cross_dimer_end_tm = 0.0f;
    bool cross_dimer_end = false;
    // --thin-panel true: after the cover / tube step the primers are thinned to those their coverage needs -- a greedy
    // set cover over "primer p has a match in segment s" within thin_mismatches mismatches, the last thin_3p_exact
    // bases exact (msspe_panel_thin; the panel of --existing-primers is forced); a pick must cover thin_min_gain new
    // segments.  The reports, the background blocks and the CSV see the thinned lists; the report gains a block.
    // The --thin-* values are read only with the switch.  "false": nothing changes.
    std::string thin_panel = "false";
    int thin_mismatches = 0;
    std::string thin_3p_exact_text = "3";
    int thin_3p_exact = 3;
    int thin_min_gain = 1;
    // --thin-depth R (with --thin-panel true): every segment keeps min(R, primers it has) primers instead of one
    // (msspe_panel_thin_depth*); a line of the block says how many segments have R.  1: nothing changes.
    int thin_depth = 1;
    // --thin-tm C (with --thin-panel true): the thinning runs over the segments a primer HOLDS at C instead -- every
    // match within thin_mismatches / thin_3p_exact scored with thal (msspe_panel_thin_thal, --thin-thal any | end1, the
    // chemistry of --coverage-tm), so the thal report of the thinned panel holds what the whole panel held.  Empty
    // text: not given, nothing changes (and --thin-thal is not read).
    std::string thin_tm_text, thin_thal;
    float thin_tm = 0.0f;
    bool thin_scored = false;
    // --select-by-coverage true: the cover / tube step of every round is replaced by one screen of the round's primers
    // with the current panel and one msspe_panel_select_packed_dev over them: the panel is forced,
    // --tubes N gives T = N (1 without it), --check-self-dimers false drop_self_pairs, --check-cross-dimers false an
    // all-zero graph; the incidence rule is --thin-panel's (--thin-mismatches, --thin-3p-exact, --thin-min-gain,
    // --thin-tm, --thin-thal, read with this switch too).  "false": nothing changes.
    std::string select_by_coverage = "false";
    // --select-depth R (with --select-by-coverage true): the selection runs on in layers, layer r adding primers for
    // the segments that still have fewer than r (msspe_panel_select_depth_packed_dev); the block's
    // first line gains ", depth R" and the thinning's "Depth:" line follows "Segments:".  1: nothing changes.
    int select_depth = 1;
    // --genome-weights <file> (with --thin-panel true at depth 1 without --thin-tm, or --select-by-coverage true at
    // depth 1): lines "name,weight" give every segment of the FASTA records of that name an integer weight >= 0, the
    // records not listed --default-genome-weight; the thinning / the selection of every round then runs on weights
    // (msspe_panel_thin_weighted_packed_dev / msspe_panel_select_weighted_packed_dev), --thin-min-gain
    // is in weight units, and the block gains a "Weight:" line behind "Segments:".  Empty: nothing changes.
    std::string genome_weights;
    int default_genome_weight = 1;
    // --primer-costs <file> / --background-site-cost <c> (with --thin-panel true without --thin-tm, or
    // --select-by-coverage true; depth 1, one device): every primer gets a cost -- its line "sequence,cost" of the file
    // (cost 1 .. 2^32 - 1, the later of two lines holds) or --default-primer-cost, plus c times its background sites
    // as --max-background-sites counts them, saturating at 2^32 - 1 -- and the thinning / the selection of every round
    // picks by gain per cost (msspe_panel_thin_cost_packed_dev / msspe_panel_select_cost_packed_dev),
    // with the weights of --genome-weights when given; the block gains a "Cost:" line.  Empty: nothing changes.  The
    // texts are read only with one of the two switches; primer_costs_on says that a cost option is in force.
    std::string primer_costs, default_primer_cost_text, background_site_cost_text;
    uint32_t default_primer_cost = 1, background_site_cost = 0;
    bool primer_costs_on = false;
    // --seed-mismatches M: a round that seeds stage A (with --existing-primers, and rounds >= 1 of --repick-rounds)
    // seeds it on what the panel COVERS -- every segment of the direction in which a panel primer has a match within M
    // mismatches, its last seed_3p_exact bases exact (msspe_kmer_candidates_both_tolerant_packed_dev) -- instead of
    // the segments that hold it verbatim, and the report gains a block per seeding round.  --seed-tm C: only the
    // matches thal scores stable at C cover (--seed-thal any | end1, the chemistry of --coverage-tm); it implies
    // M = 0 when --seed-mismatches is not given.  -1 / empty: not given -- exact seeding, nothing changes.  The values
    // are read only when a round can seed; --seed-thal needs --seed-tm; one device.
    int seed_mismatches = -1;
    std::string seed_3p_exact_text;   // empty: not given (3)
    int seed_3p_exact = 3;
    std::string seed_tm_text, seed_thal;
    float seed_tm = 0.0f;
    bool seed_scored = false, seed_tolerant = false;
    // --background FASTA: after the coverage report, the off-target sites of every kept primer in these records (both
    // strands, up to background_mismatches mismatches, the last background_3p_exact bases exact:
    // msspe_background_sites); with max_background_sites >= 0 candidates with more sites are dropped before the
    // cross-dimer screen.  Empty: nothing changes.  -1 = not given (resolved to 2 / 3 / no limit by parse()).
    std::string background;
    int background_mismatches = -1, background_3p_exact = -1, max_background_sites = -1;
    // --background-tm C: every site is scored with thal against the strand the primer would anneal to
    // (msspe_background_thal, --background-thal any | end1, the cross-dimer screen's chemistry); a site is stable iff
    // round_fixed_f32(max(0, t), 2) >= C, the report adds the stable counts and max_background_sites compares those.
    // Empty text: not given, nothing changes.
    std::string background_tm_text, background_thal;
    float background_tm = 0.0f;
    bool background_scored = false;
    // --background-amplicon-max LEN (with --background and --background-tm): after the scored block, the off-target
    // amplicons -- pairs of stable sites that face each other in one record, product length (both primers included)
    // in [background_amplicon_min, LEN] (msspe_background_amplicons; the minimum defaults to the k-mer size).  Report
    // only.  -1 = not given, nothing changes.
    int background_amplicon_max = -1, background_amplicon_min = -1;
    // --background-flank F (with --background and --background-tm): the template oligo of every scored site takes up
    // to F base columns on either side of the window (dangling ends; msspe_background_thal_flank, 0..4,
    // kmer_size + 2 F <= 32).  -1 = not given (resolved to 0 by parse()): nothing changes.
    int background_flank = -1;
    // --reach D: after everything else, a report on the run's own input genomes (each row without its gap columns):
    // the columns within D bases downstream of a site of the CSV's primers on either strand, and every genome's
    // longest stretch nothing primes into (msspe_stream_reach).  Sites: within reach_mismatches mismatches, the last
    // reach_3p_exact bases exact; with --reach-tm C only those thal (--reach-thal any | end1) scores stable at C.
    // --reach-out FILE: one CSV line per genome.  Report only.  Empty text / -1 = not given, nothing changes.
    std::string reach_text, reach_tm_text, reach_thal, reach_out;
    long long reach = -1;
    int reach_mismatches = -1, reach_3p_exact = -1;
    float reach_tm = 0.0f;
    bool reach_scored = false;
    // --thin-reach true (with --reach D): after everything else, the primers the CSV would get are thinned to those
    // the reach needs -- a greedy set cover over the columns each primer's sites reach, under --reach's site rule
    // (msspe_panel_thin_reach); a pick must reach at least thin_reach_min_gain columns nothing kept reaches yet.  The
    // --existing-primers panel is forced.  "Target reach" and --reach-out then describe the kept primers.
    std::string thin_reach = "false";
    int thin_reach_min_gain = 1;
    bool stddev_population = false;  // crate std-dev 0.1.0's divisor is unpinned
    static Args parse(int argc, const char *const *argv);   // throws UsageError
    static std::string usage();
};

struct PrimerConfig {   // config.rs:150-158
    int kmer_size;
    float min_tm, max_tm, max_self_dimer_any_tm, max_self_dimer_end_tm, max_hairpin_tm;
};

struct ProgramConfig {   // config.rs:160-177
    int max_iterations, max_mismatch_segments;
    bool keep_all, check_cross_dimers, check_self_dimers, check_hairpin;
    float tm_stddev;
    bool disable_tm_stddev, disable_min_max_tm;
    PrimerConfig primer_config;
    bool stddev_population;
};

struct SequenceRecord {   // main.rs:21-24
    std::string name, sequence;
};
std::vector<SequenceRecord> to_records(const std::string &fasta);   // main.rs:108-122
std::vector<SequenceRecord> to_records(const char *fasta, size_t size);
std::string reverse_complement(const std::string &s);               // main.rs:148-161
bool ntthal_pair_sent(const std::string &a, const std::string &b, const ProgramConfig &cfg);   // delta_g.rs:64-73
std::string format_ntthal_input(const std::vector<std::string> &primers, const ProgramConfig &cfg);   // delta_g.rs:61-81

struct KmerFrequency {   // main.rs:47-51
    std::string word;
    uint8_t direction;
    size_t frequency;
};

struct PrimerInfo {   // primer.rs:8-15 (values as od-msspe reads them back: text -> f32)
    std::string id;
    float tm = 0, gc = 0, self_any_th = 0, self_end_th = 0, hairpin_th = 0;
};

struct KmerStat {   // main.rs:67-80
    std::string word;
    uint8_t direction;
    float gc_percent, mean, std, tm;
    bool tm_ok;
    float self_any_th, self_end_th, hairpin_th;
    bool runs;
};

struct NtthalOptions {   // delta_g.rs:18-25
    float mv, dv, dntp, conc, t, dg;
    bool use_end = false;   // --max-cross-dimer-end-tm: the 3'-end rule beside the dG rule (msspe_conflict_rule)
    float end_tm = 0.0f;
    std::string *kinds_text = nullptr;   // ... and where a screen under both rules leaves its line for stdout
};

// Conflict relation produced by the cross-dimer stage: the reference's string-keyed GraphDB
// (graphdb.rs) restricted to what main.rs:754-771 consumes.
struct ConflictGraph {
    std::vector<std::string> nodes;                       // unique primer words, first-seen order
    std::map<std::string, std::set<std::string>> edges;   // directed: a -> {b : dG(a,b) < threshold}
};

class Engine {   // owns one msspe_ctx, or a group of them (one per device of --devices)
public:
    Engine(int device, const std::string &params_path);
    Engine(const std::vector<int> &devices, const std::string &params_path);
    ~Engine();
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    msspe_ctx *ctx() const { return ctx_; }         // with a group: member 0 (stage A, the coverage report)
    msspe_group *group() const { return group_; }   // nullptr: one device
    [[noreturn]] void fail(int rc) const;
    [[noreturn]] void fail_group(int rc) const;

private:
    msspe_ctx *ctx_ = nullptr;
    msspe_group *group_ = nullptr;
};

// The alignment as the device sees it: one rectangular byte matrix (rows shorter than the longest
// padded with '-'), copied to the GPU once and read by both directions of stage A and by the
// coverage report.
class DeviceAlignment {
public:
    DeviceAlignment(Engine &eng, const std::vector<SequenceRecord> &records);
    ~DeviceAlignment();
    DeviceAlignment(const DeviceAlignment &) = delete;
    DeviceAlignment &operator=(const DeviceAlignment &) = delete;
    const uint64_t *device() const { return static_cast<const uint64_t *>(dev_); }   // packed rows (msspe_device_put_rows_packed)
    int rows() const { return rows_; }
    size_t length() const { return len_; }

private:
    Engine &eng_;
    void *dev_ = nullptr;
    int rows_ = 0;
    size_t len_ = 0;
};

// main.rs:331-406 (+ :196-255): winners of one direction, in selection order
std::vector<KmerFrequency> find_candidates_kmers(Engine &eng, const std::vector<SequenceRecord> &records,
                                                 uint8_t direction, const ProgramConfig &cfg,
                                                 int segment_size, int overlap_size, int window_size);
// seed_f / seed_r (a panel being extended): words stage A takes as already picked, per direction;
// excl_f / excl_r: words it must never pick
std::pair<std::vector<KmerFrequency>, std::vector<KmerFrequency>> find_candidates_kmers_both(
    Engine &eng, const DeviceAlignment &aln, const ProgramConfig &cfg, int segment_size, int overlap_size, int window_size,
    const std::vector<std::string> &seed_f = {}, const std::vector<std::string> &seed_r = {},
    const std::vector<std::string> &excl_f = {}, const std::vector<std::string> &excl_r = {},
    const msspe_seed_rule *rule = nullptr, size_t *seed_covered = nullptr);
// rule (--seed-mismatches / --seed-tm): the seeds cover what they match under it (a tolerant seeded run);
// seed_covered[2]: the segments each direction's seeds covered before the first iteration.
// "Seeding (up to M mismatches, last E bases exact[; thal NAME, t >= T C]):" and, per direction, the segments the panel
// primers covered of the alignment's; mode 0: the match rule alone
std::string seed_report(int max_mismatches, int exact_3p, int mode, float tm_threshold, size_t covered_f, size_t panel_f,
                        size_t covered_r, size_t panel_r, size_t segments);
// --existing-primers (and --exclude-primers: `option` names the switch in the messages): the F and R primers of a
// panel CSV (the header names the columns; direction and primers are read, the others ignored); throws UsageError
// naming the line when a primer is not kmer_size bases of ACGT or the direction is not F / R
std::pair<std::vector<std::string>, std::vector<std::string>> read_panel(const std::string &path, int kmer_size,
                                                                         const char *option = "--existing-primers");
std::vector<KmerFrequency> find_candidates_kmers(Engine &eng, const DeviceAlignment &aln, uint8_t direction,
                                                 const ProgramConfig &cfg, int segment_size,
                                                 int overlap_size, int window_size);
// primer.rs:143-166
std::vector<PrimerInfo> check_primers(Engine &eng, const std::vector<std::string> &primers);
// main.rs:408-455, :462-471, :478-490, :492-516
std::vector<KmerStat> get_kmer_stats(Engine &eng, const std::vector<KmerFrequency> &kmers,
                                     const ProgramConfig &cfg);
void get_tm_stat(const std::vector<PrimerInfo> &info, bool population, float &mean, float &std);
bool tm_in_threshold(float tm, float mean, float std, float diff);
bool is_run(const std::string &kmer);
std::vector<KmerStat> filter_kmers(const std::vector<KmerStat> &stats, const ProgramConfig &cfg);
// delta_g.rs:61-153
ConflictGraph run_ntthal(Engine &eng, const std::vector<std::string> &primers,
                         const NtthalOptions &opts, const ProgramConfig &cfg);
// main.rs:754-798: primers removed by the greedy vertex cover
std::set<std::string> vertex_cover(const std::vector<std::string> &primers, const ConflictGraph &g);
// --cover-on-device true: run_ntthal + vertex_cover as one msspe_conflict_cover call over the distinct primers (the
// screen's bitmap and the cover stay on the device); the same set
std::set<std::string> conflict_cover_on_device(Engine &eng, const std::vector<std::string> &primers,
                                               const NtthalOptions &opts, const ProgramConfig &cfg);
// --tubes (engine extension): the sequential rule of DESIGN.md 4.9 over the distinct primers -- by descending
// (neighbours other than itself, lexicographic rank) each takes the lowest of max_tubes tubes that holds no neighbour
// placed before it; -1: in no tube (a self conflict, or a neighbour in every tube).  The device's independent twin.
std::map<std::string, int> assign_tubes(const std::vector<std::string> &primers, const ConflictGraph &g, int max_tubes);
// the same assignment as one msspe_conflict_tubes call over the distinct primers (the screen's bitmap stays on the
// device)
std::map<std::string, int> conflict_tubes_on_device(Engine &eng, const std::vector<std::string> &primers,
                                                    const NtthalOptions &opts, const ProgramConfig &cfg, int max_tubes);
// "Tube assignment (up to N tubes):", the tubes in use, primers per tube (CSV rows) and primers in no tube
std::string tubes_report(const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                         const std::map<std::string, int> &tubes, int max_tubes);
// --thin-panel (engine extension): the sequential rule of DESIGN.md 4.10 over incidence rows -- rows[p] holds one bit
// per segment (bit s & 63 of word s >> 6).  Forced primers cover first and are never picked; every round picks the
// unforced, unpicked primer with the most uncovered segments (ties: the lowest index) until that gain is below
// min_gain.  The device's independent twin.
struct ThinResult {
    std::vector<int> order, gains;   // the picks in order
    std::vector<char> keep;          // forced or picked
    size_t covered_all = 0, covered_kept = 0;
};
ThinResult thin_panel(const std::vector<std::vector<uint64_t>> &rows, int min_gain, const std::vector<char> &forced);
// --genome-weights (engine extension): the same rules on a weight per segment (weights[s] for bit s of a
// row, 0 past its end): a gain is the sum of the new segments' weights, min_gain is in weight units.  The gains are
// weights and go to sums.gains (the result's own gains stay empty); weight_all / weight_kept: the weight of the
// segments covered by all rows and by the kept ones.  covered_all / covered_kept stay counts of segments.  The
// device's independent twins.
struct WeightedSums {
    std::vector<uint32_t> gains;
    uint64_t weight_all = 0, weight_kept = 0;
};
ThinResult thin_panel_weighted(const std::vector<std::vector<uint64_t>> &rows, const std::vector<uint32_t> &weights,
                               long long min_gain, const std::vector<char> &forced, WeightedSums &sums);
// "  Weight:   covered A/T by all Y, K/T by the kept X": the line a weighted block carries behind "  Segments:"
std::string weight_line(uint64_t weight_all, uint64_t weight_kept, uint64_t weight_total, size_t n_all, size_t n_kept);
// --genome-weights: a weight per record from lines "name,weight" (records not listed: default_weight).  A line that is
// not "name,weight" with an integer weight in 0 .. 2^32 - 1, a name no record carries, and a total over the records'
// `partitions` segments each above 2^32 - 1 are usage errors that name the line.
std::vector<uint32_t> read_genome_weights(const std::string &path, const std::vector<SequenceRecord> &records,
                                          int default_weight, size_t partitions);
// --thin-depth (engine extension): the sequential rule of DESIGN.md 4.15 over incidence rows (as thin_panel's).
// shadow[p]: p repeats a word of its direction and counts in nothing (thin_shadows marks them: among equal words all
// but the forced one of lowest index, or without a forced one the lowest index).  Every segment needs
// min(depth, representatives that match it); forced representatives count first; every round picks the live
// representative matching the most open segments (ties: the lowest index) until that gain is below min_gain.
// depth_all / depth_kept: representatives per segment among all and among the kept, saturating at 255; counts:
// segments with depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >= depth.  The device's independent
// twin, every round from scratch.
struct ThinDepthResult {
    std::vector<int> order, gains;
    std::vector<char> keep;          // forced (shadows included) or picked
    std::vector<uint8_t> depth_all, depth_kept;
    long long counts[4] = {0, 0, 0, 0};
    int rounds = 0;                  // the picks and the one that stopped
};
std::vector<char> thin_shadows(const std::vector<std::string> &fwd, const std::vector<std::string> &rev,
                               const std::vector<char> &forced);
ThinDepthResult thin_panel_depth(const std::vector<std::vector<uint64_t>> &rows, size_t n_seg, int depth, int min_gain,
                                 const std::vector<char> &forced, const std::vector<char> &shadow);
// --select-by-coverage (engine extension): the sequential rule of DESIGN.md 4.13 over incidence rows (as thin_panel's)
// and the cover's graph over primers[p] (symmetric; an edge a -> a is a self conflict).  Forced primers cover first,
// are never picked, and bar their neighbours from every tube; every round picks the live primer (not kept, not
// self-conflicting, a tube in [0, max_tubes) left) with the most uncovered segments, ties to the lowest index, gives it
// the lowest tube its neighbours left and bars them from that tube, until that gain is below min_gain.  The device's
// independent twin.
struct SelectResult {
    std::vector<int> order, gains;   // the picks in order
    std::vector<char> keep;          // forced or picked
    std::vector<int> tube;           // of a pick; -1 for everyone else
    std::vector<char> barred;        // not kept, and self-conflicting or no tube left at the end
    std::vector<uint64_t> covered;   // by the kept, bit s & 63 of word s >> 6
    size_t covered_all = 0, covered_kept = 0;
    int tubes_used = 0, rounds = 0;  // rounds: the picks and the one that stopped
};
SelectResult select_panel(const std::vector<std::vector<uint64_t>> &rows, const std::vector<std::string> &primers,
                          const ConflictGraph &g, int max_tubes, int min_gain, const std::vector<char> &forced);
// select_panel on a weight per segment: thin_panel_weighted's conventions (sums.gains, weight_all, weight_kept)
SelectResult select_panel_weighted(const std::vector<std::vector<uint64_t>> &rows,
                                   const std::vector<std::string> &primers, const ConflictGraph &g,
                                   const std::vector<uint32_t> &weights, int max_tubes, long long min_gain,
                                   const std::vector<char> &forced, WeightedSums &sums);
// --primer-costs / --background-site-cost (engine extension): the rules of thin_panel and select_panel with the pick by
// gain per cost.  costs[p] >= 1, one per row.  weights (optional): a weight per segment as in the
// weighted twins; without them a gain is a count.  A round considers the live primers whose gain is at least min_gain
// and picks the greatest gain / cost -- by 64-bit cross products, never a division -- then the greater gain, then the
// lowest index.  The gains go to sums.gains (the result's own gains stay empty); without weights weight_all /
// weight_kept are the two covered counts; cost_all / cost_kept: the costs' sum over all rows and over the kept ones.
// The device's independent twins, every round from scratch.
struct CostSums {
    std::vector<uint32_t> gains;
    uint64_t weight_all = 0, weight_kept = 0, cost_all = 0, cost_kept = 0;
};
ThinResult thin_panel_cost(const std::vector<std::vector<uint64_t>> &rows, const std::vector<uint32_t> *weights,
                           const std::vector<uint32_t> &costs, long long min_gain, const std::vector<char> &forced,
                           CostSums &sums);
SelectResult select_panel_cost(const std::vector<std::vector<uint64_t>> &rows, const std::vector<std::string> &primers,
                               const ConflictGraph &g, const std::vector<uint32_t> *weights,
                               const std::vector<uint32_t> &costs, int max_tubes, long long min_gain,
                               const std::vector<char> &forced, CostSums &sums);
// "  Cost:     K/A by the kept m of n": the line a block carries behind "  Segments:" (behind "  Weight:" when present).
// K and A are the costs of the kept primers and of all primers of the call, m and n their numbers; the panel's forced
// primers count in all four.
std::string cost_line(uint64_t cost_kept, uint64_t cost_all, size_t n_kept, size_t n_all);
// --primer-costs: a cost per primer sequence from lines "sequence,cost".  A line that is not "sequence,cost" with
// kmer_size bases A/C/G/T and an integer cost in 1 .. 2^32 - 1 is a usage error that names the line; a sequence listed
// twice takes the later line.
std::map<std::string, uint32_t> read_primer_costs(const std::string &path, int kmer_size);
// base + per_site * sites, saturating at 2^32 - 1 (--background-site-cost)
uint32_t primer_cost(uint32_t base, uint32_t per_site, uint64_t sites);
// the costs of a list of primers, in its order: what the thinning and the selection ask for the lists they see
using PrimerCostFn = std::function<std::vector<uint32_t>(const std::vector<std::string> &words)>;
// --select-depth R (engine extension): the layered rule of DESIGN.md 4.16 over the same rows and graph, n_seg segments
// (bits of a row).  cnt[s] = kept primers that match s, from the forced rows on; layers r = 1 .. min(R, max(1, deepest
// segment)): in layer r a segment is open while cnt < min(r, primers that match it), a round picks the live primer
// matching the most open segments (ties: the lowest index) and counts it on every segment it matches, until that gain
// is below min_gain; barring, picks and cnt carry over.  Layer 1 is select_panel.  The device's independent twin.
struct SelectDepthResult {
    std::vector<int> order, gains, layer;   // the picks in order, each with its gain and its layer
    std::vector<char> keep;
    std::vector<int> tube;
    std::vector<char> barred;
    std::vector<uint8_t> depth_all, depth_kept;   // saturating at 255
    long long counts[4] = {0, 0, 0, 0};           // as ThinDepthResult's
    int tubes_used = 0, rounds = 0, layers = 0;   // rounds: the picks and every layer's stopping round
};
SelectDepthResult select_panel_depth(const std::vector<std::vector<uint64_t>> &rows,
                                     const std::vector<std::string> &primers, const ConflictGraph &g, size_t n_seg,
                                     int depth, int max_tubes, int min_gain, const std::vector<char> &forced);
// the same rule on the device for one round of the CLI: the round's primers (fwd / rev, stage B's survivors) and the
// current panel (forced) are screened as one pool (msspe_cross_dimer_dev, bitmap only; screen false: no edges) and
// selected by one msspe_panel_select_packed_dev.  The kept primers are appended to kept_f / kept_r in their lists'
// order with their tubes in `tubes`; dropped(primer, barred) is called for every other one.  A word met a second time
// (the other direction's list, the panel) is not offered.  Returns select_report's block.  genome_weights
// (--genome-weights: a weight per row of the alignment, depth 1): msspe_panel_select_weighted_packed_dev instead, and
// the block carries weight_line behind "Segments:".
std::string select_panel_on_device(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                                   const std::vector<KmerStat> &rev, const std::vector<std::string> &panel_f,
                                   const std::vector<std::string> &panel_r, int segment_size, int overlap_size,
                                   int window_size, int kmer_size, int max_mismatches, int exact_3p, int min_gain,
                                   const msspe_chem &chem, int mode, float tm_threshold, int max_tubes, bool list_tubes,
                                   bool screen, bool drop_self_pairs, float dg_threshold, std::vector<KmerStat> &kept_f,
                                   std::vector<KmerStat> &kept_r, std::map<std::string, int> &tubes,
                                   const std::function<void(const KmerStat &, bool)> &dropped,
                                   const NtthalOptions *end_rule = nullptr, int depth = 1,
                                   const std::vector<uint32_t> *genome_weights = nullptr,
                                   const PrimerCostFn *costs = nullptr);
// "Panel selection by coverage (<the match rule>, gain >= G, tubes <= T):", the rule line, the primers kept of those
// offered (forced ones apart), the primers barred, the segments covered (mode 0) or held (modes 1, 2) by all of them
// and by the kept ones, and with per_tube the primers per tube; depth above 1 (--select-depth R): ", depth R" closes
// the first line's bracket and thin_report's "Depth:" line follows "Segments:" (deep_all = u, deep_kept = v)
std::string select_report(int mode, float tm_threshold, int max_mismatches, int exact_3p, int min_gain, int max_tubes,
                          size_t kept_f, size_t n_f, size_t kept_r, size_t n_r, size_t forced, size_t barred,
                          size_t covered_all, size_t covered_kept, size_t segments,
                          const std::vector<size_t> *per_tube, int depth = 1, size_t deep_all = 0,
                          size_t deep_kept = 0);
// the same rule as one msspe_panel_thin_packed_dev call on the resident alignment: fwd / rev are thinned in place,
// the panel's primers are forced; returns the report's block.  genome_weights (--genome-weights: a weight per row of
// the alignment; depth 1, no chemistry): msspe_panel_thin_weighted_packed_dev instead, and the block carries weight_line
std::string thin_panel_on_device(Engine &eng, const DeviceAlignment &aln, std::vector<KmerStat> &fwd,
                                 std::vector<KmerStat> &rev, const std::vector<std::string> &panel_f,
                                 const std::vector<std::string> &panel_r, int segment_size, int overlap_size,
                                 int window_size, int kmer_size, int max_mismatches, int exact_3p, int min_gain,
                                 const msspe_chem *chem = nullptr, int mode = 1, float tm_threshold = 0.0f,
                                 int depth = 1, const std::vector<uint32_t> *genome_weights = nullptr,
                                 const PrimerCostFn *costs = nullptr);
// costs (--primer-costs / --background-site-cost; depth 1, no chemistry): msspe_panel_thin_cost_packed_dev /
// msspe_panel_select_cost_packed_dev instead, with the weights when given, and the block carries cost_line
// depth above 1 (--thin-depth R): msspe_panel_thin_depth_packed_dev / msspe_panel_thin_thal_depth_packed_dev instead;
// the block's first line gains ", depth R" and a line "  Depth:    at least R primers on u/t segments by all Y, on
// v/t by the kept X" follows "Segments:" (thin_report / thin_thal_report with depth, deep_all = u, deep_kept = v).
// with a chemistry (--thin-tm) thin_panel_on_device calls msspe_panel_thin_thal_packed_dev and returns this block:
// "Panel thinning (thal NAME, t >= T C; matches within M mismatches, last E bases exact, gain >= G):", the primers
// kept as in thin_report, and the segments held by all of them and by the kept ones
std::string thin_thal_report(int mode, float tm_threshold, int max_mismatches, int exact_3p, int min_gain,
                             size_t kept_f, size_t n_f, size_t kept_r, size_t n_r, size_t forced, size_t held_all,
                             size_t held_kept, size_t segments, int depth = 1, size_t deep_all = 0,
                             size_t deep_kept = 0);
// "Panel thinning (up to M mismatches, last E bases exact, gain >= G):", the primers kept of those offered (forced
// ones apart) and the segments covered by all of them and by the kept ones (forced primers cover in both figures)
std::string thin_report(int max_mismatches, int exact_3p, int min_gain, size_t kept_f, size_t n_f, size_t kept_r,
                        size_t n_r, size_t forced, size_t covered_all, size_t covered_kept, size_t segments,
                        int depth = 1, size_t deep_all = 0, size_t deep_kept = 0);
// main.rs:518-594 (text goes to `out`): the per-segment search runs on the device
// (msspe_segment_coverage_dev), the totals per sequence / partition and the text on the host
std::string coverage_report(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                            const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                            int segment_size, int overlap_size, int window_size, int kmer_size);
std::string coverage_report(Engine &eng, const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                            const std::vector<SequenceRecord> &records, int segment_size,
                            int overlap_size, int window_size, int kmer_size);
// The thal-scored block (engine extension, --coverage-tm): "Coverage report (thal NAME, t >= T C; matches within M
// mismatches, last E bases exact):", the segments held / matched, the sequences at >= 80 % held and the primers that
// hold no segment.  coverage_thal_block is the text alone, from held[record * P + partition] (0 / 1 / 2) and the
// per-primer held counts (msspe_segment_coverage_thal); coverage_report_thal makes both on the device first.
std::string coverage_thal_block(const std::vector<SequenceRecord> &records, size_t P, int segment_size,
                                int overlap_size, const uint8_t *held, const uint32_t *primer_held, size_t n_primers,
                                int max_mismatches, int exact_3p, int mode, float tm_threshold);
std::string coverage_report_thal(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                                 const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                                 int segment_size, int overlap_size, int window_size, int kmer_size, int max_mismatches,
                                 int exact_3p, const msspe_chem &chem, int mode, float tm_threshold);
// The mismatch-tolerant block (engine extension): "Coverage report (up to N mismatches, last E bases exact):", the
// exact report's three lines with hit = best <= N, and the segments by best mismatch count (msspe_segment_coverage_mm)
std::string coverage_report_mm(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                               const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                               int segment_size, int overlap_size, int window_size, int kmer_size, int max_mismatches,
                               int exact_3p);
std::string coverage_report_mm(Engine &eng, const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                               const std::vector<SequenceRecord> &records, int segment_size, int overlap_size,
                               int window_size, int kmer_size, int max_mismatches, int exact_3p);
// --background (engine extension): the records as one packed stream on the device, uploaded once
class DeviceBackground {
public:
    DeviceBackground(Engine &eng, const std::vector<SequenceRecord> &records);
    ~DeviceBackground();
    DeviceBackground(const DeviceBackground &) = delete;
    DeviceBackground &operator=(const DeviceBackground &) = delete;
    // (plus, minus) sites of each word, one msspe_background_sites_packed_dev call per word length
    std::vector<std::pair<uint64_t, uint64_t>> sites(const std::vector<std::string> &words, int max_mismatches,
                                                     int exact_3p) const;
    // the same with the thal score of every site (one msspe_background_thal_packed_dev call per word length):
    // returns the (plus, minus) sites, stable_out the (plus, minus) stable ones.  flank > 0: the _flank calls; a
    // length class of k bases is scored with min(flank, (32 - k) / 2), the widest flank its template oligo has room for
    std::vector<std::pair<uint64_t, uint64_t>> scored(const std::vector<std::string> &words, int max_mismatches,
                                                      int exact_3p, const msspe_chem &chem, int mode,
                                                      float tm_threshold,
                                                      std::vector<std::pair<uint64_t, uint64_t>> &stable_out,
                                                      int flank = 0) const;
    // scored() and, from the same pass, the off-target amplicons of the words' stable sites (one
    // msspe_background_amplicons_packed_dev call per word length on the resident stream; primers of different lengths
    // are not paired): amplicons_out (as forward, as reverse) per word; list_out: every amplicon, fwd and rev indices
    // into words, sorted by (pos, len, fwd, rev)
    std::vector<std::pair<uint64_t, uint64_t>> amplicons(const std::vector<std::string> &words, int max_mismatches,
                                                         int exact_3p, const msspe_chem &chem, int mode,
                                                         float tm_threshold, uint32_t min_len, uint32_t max_len,
                                                         std::vector<std::pair<uint64_t, uint64_t>> &stable_out,
                                                         std::vector<std::pair<uint64_t, uint64_t>> &amplicons_out,
                                                         std::vector<msspe_amplicon> &list_out, int flank = 0) const;
    // (record id, offset in the record) of stream position pos
    std::pair<std::string, uint64_t> locate(uint64_t pos) const;
    // msspe_stream_reach_packed_dev on the resident stream with its own record starts, flank 0: n packed words of k
    // bases; counts / stable hold 2 n entries, out one per record.  Returns the status.
    int reach(int k, const msspe_mismatch_opt &mm, const std::vector<uint64_t> &packed, int n, const msspe_chem &chem,
              int mode, float tm_threshold, const msspe_reach_opt &opt, std::vector<uint64_t> &counts,
              std::vector<uint64_t> &stable, std::vector<msspe_reach_record> &out) const;
    // msspe_panel_thin_reach_packed_dev likewise: forced / keep hold n flags, order / gains n entries; out describes
    // the kept primers.  Returns the status.
    int thin_reach(int k, const msspe_mismatch_opt &mm, const std::vector<uint64_t> &packed, int n,
                   const msspe_chem &chem, int mode, float tm_threshold, const msspe_reach_opt &opt, int min_gain,
                   const std::vector<uint8_t> &forced, std::vector<uint8_t> &keep, std::vector<uint32_t> &order,
                   std::vector<uint32_t> &gains, int &n_picked, long long &reached_all, long long &reached_kept,
                   std::vector<uint64_t> &counts, std::vector<uint64_t> &stable,
                   std::vector<msspe_reach_record> &out) const;

private:
    Engine &eng_;
    void *dev_ = nullptr;
    size_t len_ = 0;
    std::vector<std::string> names_;   // of the records, and their first stream columns: locate()
    std::vector<uint64_t> starts_;
};
// "Background sites (up to M mismatches, last E bases exact):", one line per primer (name as in the CSV, plus-strand
// and minus-strand sites) and a totals line
std::string background_report(const std::vector<std::string> &names,
                              const std::vector<std::pair<uint64_t, uint64_t>> &sites, int max_mismatches,
                              int exact_3p);
// The block with --background-tm: the heading names the rule ("; stable: thal ANY t >= 30.00 C"), every line and the
// totals add "stable plus S, minus T"; flank > 0 appends ", template flank F" behind the threshold
std::string background_report_scored(const std::vector<std::string> &names,
                                     const std::vector<std::pair<uint64_t, uint64_t>> &sites,
                                     const std::vector<std::pair<uint64_t, uint64_t>> &stable, int max_mismatches,
                                     int exact_3p, int mode, float tm_threshold, int flank = 0);
// "Background amplicons (stable sites facing each other, MIN to MAX bases):", one line per primer (amplicons as
// forward and as reverse), a totals line and the first 20 amplicons of the sorted list as
// "record:offset, length, forward name, reverse name"
std::string background_report_amplicons(const std::vector<std::string> &names,
                                        const std::vector<std::pair<uint64_t, uint64_t>> &counts,
                                        const std::vector<msspe_amplicon> &list, const DeviceBackground &background,
                                        uint32_t min_len, uint32_t max_len);
// --thin-reach: what the thinning takes (min_gain, one forced flag per word) and gives (one keep flag per word, the
// columns all words and the kept words reach)
struct ReachThinning {
    int min_gain = 1;
    std::vector<uint8_t> forced, keep;
    long long reached_all = 0, reached_kept = 0;
};
// --reach (engine extension): the input rows without their gap columns (genomes_out) as one resident stream, screened
// with `words` (all of k bases) on both strands; one record per genome, positions in that stream.  With thin the same
// pass thins the words on reach, and the records describe the kept words.
std::vector<msspe_reach_record> target_reach(Engine &eng, const std::vector<SequenceRecord> &records,
                                             const std::vector<std::string> &words, int k, int max_mismatches,
                                             int exact_3p, const msspe_chem &chem, int mode, float tm_threshold,
                                             uint32_t reach, std::vector<std::string> &genomes_out,
                                             ReachThinning *thin = nullptr);
// "Reach thinning (extension D bases, min gain G; sites: ...):", kept of n primers with the forced ones, and the columns
// all primers and the kept primers reach
std::string reach_thinning_report(const ReachThinning &thin, uint32_t reach, int max_mismatches, int exact_3p,
                                  bool scored, int mode, float tm_threshold);
// "Target reach (extension D bases; sites: ...):", the totals over all genomes, the number of genomes whose longest gap
// (columns reached on neither strand) exceeds D, and the 20 genomes with the longest such gap as "name: offset, length"
std::string target_reach_report(const std::vector<std::string> &names, const std::vector<std::string> &genomes,
                                const std::vector<msspe_reach_record> &recs, uint32_t reach, int max_mismatches,
                                int exact_3p, bool scored, int mode, float tm_threshold);
// --reach-out: a header and one line per genome with every field, positions as offsets in the ungapped genome
std::string target_reach_csv(const std::vector<std::string> &names, const std::vector<std::string> &genomes,
                             const std::vector<msspe_reach_record> &recs);
// main.rs:834-858
// first_f / first_r: the number of the first row of each direction (a panel's extension continues its numbering)
// tubes (--tubes): an eighth column "tube", 1-based, empty for a primer in no tube
std::string primers_csv(const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev, size_t first_f = 0,
                        size_t first_r = 0, const std::map<std::string, int> *tubes = nullptr);

// main.rs:596-861 without the MAFFT call: returns the process exit code; report -> stdout
int run(const Args &args, std::string &stdout_text);

}  // namespace od_msspe
