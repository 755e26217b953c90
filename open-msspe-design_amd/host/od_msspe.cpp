// od_msspe.cpp -- see od_msspe.hpp.  Mirrors /root/reference/od-msspe/src/main.rs, primer.rs,
// delta_g.rs and config.rs for the hot path and its immediate callers; all arithmetic of the hot
// path happens in libmsspe_hip.so.
#include "od_msspe.hpp"

#include <algorithm>
#include <array>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <thread>

#include <fcntl.h>
#include <spawn.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <unordered_set>

extern char **environ;

namespace od_msspe {

// ---------------------------------------------------------------------------------------------
// CLI (config.rs:11-148)
// ---------------------------------------------------------------------------------------------
namespace {

struct OptSpec {
    const char *flag, *env;
    enum Kind { Int, OptInt, Float, Bool, Str } kind;
    size_t offset;
};
#define OFF(f) offsetof(Args, f)
const OptSpec kOpts[] = {
    {"--kmer-size", "KMER_SIZE", OptSpec::Int, OFF(kmer_size)},
    {"--window-size", "WINDOW_SIZE", OptSpec::Int, OFF(window_size)},
    {"--overlap-size", "OVERLAP_SIZE", OptSpec::Int, OFF(overlap_size)},
    {"--max-mismatch-segments", "MAX_MISMATCH_SEGMENTS", OptSpec::OptInt, OFF(max_mismatch_segments)},
    {"--max-iterations", "MAX_ITERATIONS", OptSpec::Int, OFF(max_iterations)},
    {"--search-windows-size", "SEARCH_WINDOWS_SIZE", OptSpec::Int, OFF(search_windows_size)},
    {"--mv-conc", "MV_CONC", OptSpec::Float, OFF(mv_conc)},
    {"--dv-conc", "DV_CONC", OptSpec::Float, OFF(dv_conc)},
    {"--dntp-conc", "DNTP_CONC", OptSpec::Float, OFF(dntp_conc)},
    {"--dna-conc", "DNA_CONC", OptSpec::Float, OFF(dna_conc)},
    {"--annealing-temp", "ANNEALING_TEMP", OptSpec::Float, OFF(annealing_temp)},
    {"--min-tm", "MIN_TM", OptSpec::Float, OFF(min_tm)},
    {"--max-tm", "MAX_TM", OptSpec::Float, OFF(max_tm)},
    {"--max-self-dimer-any-tm", "MAX_SELF_DIMER_ANY_TM", OptSpec::Float, OFF(max_self_dimer_any_tm)},
    {"--max-self-dimer-end-tm", "MAX_SELF_DIMER_END_TM", OptSpec::Float, OFF(max_self_dimer_end_tm)},
    {"--max-hairpin-tm", "MAX_HAIRPIN_TM", OptSpec::Float, OFF(max_hairpin_tm)},
    {"--delta-g-threshold", "DELTA_G_THRESHOLD", OptSpec::Float, OFF(delta_g_threshold)},
    {"--max-cross-dimer-end-tm", "MAX_CROSS_DIMER_END_TM", OptSpec::Str, OFF(max_cross_dimer_end_tm_text)},
    {"--keep-all", "KEEP_ALL", OptSpec::Bool, OFF(keep_all)},
    {"--check-cross-dimers", "CHECK_CROSS_DIMERS", OptSpec::Bool, OFF(check_cross_dimers)},
    {"--existing-primers", "EXISTING_PRIMERS", OptSpec::Str, OFF(existing_primers)},
    {"--exclude-primers", "EXCLUDE_PRIMERS", OptSpec::Str, OFF(exclude_primers)},
    {"--rejected-out", "REJECTED_OUT", OptSpec::Str, OFF(rejected_out)},
    {"--repick-rounds", "REPICK_ROUNDS", OptSpec::Int, OFF(repick_rounds)},
    {"--check-self-dimers", "CHECK_SELF_DIMERS", OptSpec::Bool, OFF(check_self_dimers)},
    {"--check-hairpin", "CHECK_HAIRPIN", OptSpec::Bool, OFF(check_hairpin)},
    {"--tm-stddev", "TM_STDDEV", OptSpec::Float, OFF(tm_stddev)},
    {"--disable-tm-stddev", "DISABLE_TM_STDDEV", OptSpec::Bool, OFF(disable_tm_stddev)},
    {"--disable-min-max-tm", "DISABLE_MIN_MAX_TM", OptSpec::Bool, OFF(disable_min_max_tm)},
    {"--do-align", "DO_ALIGN", OptSpec::Bool, OFF(do_align)},
    {"--ntthal", "NTTHAL", OptSpec::Str, OFF(ntthal)},
    {"--primer3", "PRIMER3", OptSpec::Str, OFF(primer3)},
    {"--params-path", "MSSPE_PARAMS_PATH", OptSpec::Str, OFF(params_path)},
    {"--device", "MSSPE_DEVICE", OptSpec::Int, OFF(device)},
    {"--devices", "MSSPE_DEVICES", OptSpec::Str, OFF(devices)},
    {"--cover-on-device", "COVER_ON_DEVICE", OptSpec::Bool, OFF(cover_on_device)},
    {"--tubes", "TUBES", OptSpec::Int, OFF(tubes)},
    {"--coverage-mismatches", "COVERAGE_MISMATCHES", OptSpec::Int, OFF(coverage_mismatches)},
    {"--coverage-3p-exact", "COVERAGE_3P_EXACT", OptSpec::Str, OFF(coverage_3p_exact_text)},
    {"--coverage-tm", "COVERAGE_TM", OptSpec::Str, OFF(coverage_tm_text)},
    {"--coverage-thal", "COVERAGE_THAL", OptSpec::Str, OFF(coverage_thal)},
    {"--thin-panel", "THIN_PANEL", OptSpec::Bool, OFF(thin_panel)},
    {"--thin-mismatches", "THIN_MISMATCHES", OptSpec::Int, OFF(thin_mismatches)},
    {"--thin-3p-exact", "THIN_3P_EXACT", OptSpec::Str, OFF(thin_3p_exact_text)},
    {"--thin-min-gain", "THIN_MIN_GAIN", OptSpec::Int, OFF(thin_min_gain)},
    {"--thin-depth", "THIN_DEPTH", OptSpec::Int, OFF(thin_depth)},
    {"--thin-tm", "THIN_TM", OptSpec::Str, OFF(thin_tm_text)},
    {"--thin-thal", "THIN_THAL", OptSpec::Str, OFF(thin_thal)},
    {"--select-by-coverage", "SELECT_BY_COVERAGE", OptSpec::Bool, OFF(select_by_coverage)},
    {"--select-depth", "SELECT_DEPTH", OptSpec::Int, OFF(select_depth)},
    {"--genome-weights", "GENOME_WEIGHTS", OptSpec::Str, OFF(genome_weights)},
    {"--default-genome-weight", "DEFAULT_GENOME_WEIGHT", OptSpec::Int, OFF(default_genome_weight)},
    {"--primer-costs", "PRIMER_COSTS", OptSpec::Str, OFF(primer_costs)},
    {"--default-primer-cost", "DEFAULT_PRIMER_COST", OptSpec::Str, OFF(default_primer_cost_text)},
    {"--background-site-cost", "BACKGROUND_SITE_COST", OptSpec::Str, OFF(background_site_cost_text)},
    {"--seed-mismatches", "SEED_MISMATCHES", OptSpec::OptInt, OFF(seed_mismatches)},
    {"--seed-3p-exact", "SEED_3P_EXACT", OptSpec::Str, OFF(seed_3p_exact_text)},
    {"--seed-tm", "SEED_TM", OptSpec::Str, OFF(seed_tm_text)},
    {"--seed-thal", "SEED_THAL", OptSpec::Str, OFF(seed_thal)},
    {"--background", "BACKGROUND", OptSpec::Str, OFF(background)},
    {"--background-mismatches", "BACKGROUND_MISMATCHES", OptSpec::OptInt, OFF(background_mismatches)},
    {"--background-3p-exact", "BACKGROUND_3P_EXACT", OptSpec::OptInt, OFF(background_3p_exact)},
    {"--max-background-sites", "MAX_BACKGROUND_SITES", OptSpec::OptInt, OFF(max_background_sites)},
    {"--background-tm", "BACKGROUND_TM", OptSpec::Str, OFF(background_tm_text)},
    {"--background-thal", "BACKGROUND_THAL", OptSpec::Str, OFF(background_thal)},
    {"--background-amplicon-max", "BACKGROUND_AMPLICON_MAX", OptSpec::OptInt, OFF(background_amplicon_max)},
    {"--background-amplicon-min", "BACKGROUND_AMPLICON_MIN", OptSpec::OptInt, OFF(background_amplicon_min)},
    {"--background-flank", "BACKGROUND_FLANK", OptSpec::OptInt, OFF(background_flank)},
    {"--reach", "REACH", OptSpec::Str, OFF(reach_text)},
    {"--reach-mismatches", "REACH_MISMATCHES", OptSpec::OptInt, OFF(reach_mismatches)},
    {"--reach-3p-exact", "REACH_3P_EXACT", OptSpec::OptInt, OFF(reach_3p_exact)},
    {"--reach-tm", "REACH_TM", OptSpec::Str, OFF(reach_tm_text)},
    {"--reach-thal", "REACH_THAL", OptSpec::Str, OFF(reach_thal)},
    {"--reach-out", "REACH_OUT", OptSpec::Str, OFF(reach_out)},
    {"--thin-reach", "THIN_REACH", OptSpec::Bool, OFF(thin_reach)},
    {"--thin-reach-min-gain", "THIN_REACH_MIN_GAIN", OptSpec::Int, OFF(thin_reach_min_gain)},
};
#undef OFF

void assign(Args &a, const OptSpec &o, const std::string &v)
{
    char *base = reinterpret_cast<char *>(&a);
    char *end = nullptr;
    switch (o.kind) {
    case OptSpec::Int:
    case OptSpec::OptInt: {
        const long x = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || x < 0)
            throw UsageError(std::string("error: invalid value '") + v + "' for '" + o.flag + "'");
        *reinterpret_cast<int *>(base + o.offset) = (int)x;
        break;
    }
    case OptSpec::Float: {
        const float x = std::strtof(v.c_str(), &end);
        if (v.empty() || *end)
            throw UsageError(std::string("error: invalid value '") + v + "' for '" + o.flag + "'");
        *reinterpret_cast<float *>(base + o.offset) = x;
        break;
    }
    case OptSpec::Bool:
        if (v != "true" && v != "false")   // config.rs value_parser = ["true", "false"]
            throw UsageError(std::string("error: invalid value '") + v + "' for '" + o.flag +
                             " <...>'\n  [possible values: true, false]");
        *reinterpret_cast<std::string *>(base + o.offset) = v;
        break;
    case OptSpec::Str:
        *reinterpret_cast<std::string *>(base + o.offset) = v;
        break;
    }
}

}  // namespace

std::string Args::usage()
{
    std::string u = "Usage: od-msspe-hip --input <INPUT> --output <OUTPUT> [OPTIONS]\n\nOptions:\n"
                    "  -i, --input <INPUT>\n  -o, --output <OUTPUT>\n";
    for (const auto &o : kOpts) u += std::string("      ") + o.flag + " <...>  [env: " + o.env + "=]\n";
    u += "      --stddev-population   divide the Tm variance by n instead of n-1\n";
    u += "\n--background <FASTA> screens the primers against unaligned background records (a host genome, rRNA) for\n"
         "off-target sites on both strands; with --devices it runs on the first device.\n"
         "--tubes <N> (1..64) splits the primers into at most N reaction tubes in which no two primers conflict, instead\n"
         "of deleting primers by the vertex cover; the CSV gains a 'tube' column. One tube is not a better cover.\n"
         "--thin-panel true drops, after the cover or the tubes, every primer the coverage does not need: a greedy set\n"
         "cover of the segments matched within --thin-mismatches <M> (last --thin-3p-exact <E> bases exact), a pick\n"
         "covering at least --thin-min-gain <G> new segments. No segment is lost at G = 1; a segment's best mismatch\n"
         "count may rise up to M. The primers of --existing-primers are kept. One device; not with --keep-all true.\n"
         "With --thin-depth <R> every segment keeps R primers where the panel has that many (a word listed twice counts\n"
         "once), and the block says how many segments have R.\n"
         "With --thin-tm <C> the cover is of the segments a primer holds at C instead: every match within M / E is scored\n"
         "with thal (--thin-thal any | end1), and no held segment is lost at G = 1; a segment's best t may fall.\n"
         "--select-by-coverage true replaces the cover (or the tube split) by a selection that looks at coverage: round\n"
         "after round the primer covering the most segments nothing kept covers yet is kept, and its conflict\n"
         "neighbours are barred (with --tubes <N>: from its tube only). With --select-depth <R> (1..255) the selection\n"
         "then runs on in layers: layer r adds primers for the segments that still have fewer than r, so a segment\n"
         "keeps up to R primers and asking for depth never costs a segment. The match rule is --thin-panel's\n"
         "(--thin-mismatches, --thin-3p-exact, --thin-min-gain, --thin-tm, --thin-thal); the primers of\n"
         "--existing-primers are kept and bar their neighbours from every tube. Conflicts may cost segments. One\n"
         "device; not with --thin-panel true, --keep-all true or --cover-on-device true.\n"
         "--genome-weights <FILE> makes --thin-panel true and --select-by-coverage true count a segment by the weight of\n"
         "its genome: lines 'name,weight' (the FASTA record's name, an integer >= 0), --default-genome-weight <W>\n"
         "(default 1) for the records not listed. A gain is the sum of the new segments' weights, --thin-min-gain is in\n"
         "weight units, genomes of weight 0 are reported but get no primer of their own, and the block gains a 'Weight:'\n"
         "line. All weights times the segments per genome may add up to 4294967295. Depth 1 only; not with --thin-panel\n"
         "true --thin-tm.\n"
         "--primer-costs <FILE> makes --thin-panel true and --select-by-coverage true pick by coverage per cost: lines\n"
         "'sequence,cost' (the primer as the CSV prints it, an integer 1 .. 4294967295; a sequence listed twice takes\n"
         "the later line), --default-primer-cost <N> (default 1) for the primers not listed. A round keeps the primer\n"
         "with the greatest new coverage divided by its cost, compared exactly; equal ratios go to the greater\n"
         "coverage. --background-site-cost <C> (needs --background) adds C times a primer's background sites, counted as\n"
         "--max-background-sites counts them, to its cost, so a clean primer is preferred to an interchangeable one\n"
         "with off-target sites. --genome-weights applies as before, and the block gains a 'Cost:' line. Depth 1 only;\n"
         "one device; not with --thin-panel true --thin-tm.\n"
         "--coverage-tm <C> adds a report of the segments the final primers hold at C: every match within\n"
         "--coverage-mismatches (last --coverage-3p-exact bases exact) is scored with thal (--coverage-thal any | end1)\n"
         "against the strand the primer anneals to. One device.\n"
         "--max-cross-dimer-end-tm <C> makes two primers conflict also when the 3' end of either anneals to the other:\n"
         "thal END1 of the ordered pair, od-msspe's SELF_END rule at C, beside the dG rule of --delta-g-threshold. The\n"
         "cover, --cover-on-device, --tubes, --select-by-coverage, --existing-primers and the later --repick-rounds all\n"
         "see the union, and stdout gains a line with the pairs of each kind. With --devices the union screen runs on\n"
         "the first device: the group has no 3'-end path.\n"
         "--exclude-primers <CSV> names words stage A must never pick (direction and primers columns, as a panel).\n"
         "--rejected-out <CSV> writes every candidate the run dropped (direction,name,primers,round,reason; reason is\n"
         "stage_b, background, panel_dimer or cover; with --select-by-coverage true select_conflict or select_unneeded in\n"
         "place of the last two); --exclude-primers reads such a file.\n"
         "--repick-rounds <N> (0..16) repeats the selection up to N times: what passed is kept as a panel, what was\n"
         "dropped is excluded, and stage A fills the holes. One device; not with --tubes.\n"
         "--seed-mismatches <M> makes a run that extends a panel (--existing-primers, and the later rounds of\n"
         "--repick-rounds) count a segment as covered already when a panel primer matches it within M mismatches, its last\n"
         "--seed-3p-exact <E> bases exact, instead of only where it occurs verbatim; with --seed-tm <C> only where thal\n"
         "(--seed-thal any | end1) scores such a match stable at C. One device.\n"
         "--reach <D> adds a report on the input genomes themselves: how much of every genome lies within D bases\n"
         "downstream of a site of the primers the CSV gets (the extension product, the primer included), on either\n"
         "strand, and where its longest stretch lies that nothing primes into. Sites are matches within\n"
         "--reach-mismatches <M> (default 2), the last --reach-3p-exact <E> bases exact (default 3); with --reach-tm <C>\n"
         "only those thal (--reach-thal any | end1) scores stable at C. --reach-out <FILE> writes one CSV line per\n"
         "genome. Needs --kmer-size 2..31; with --devices it runs on the first device.\n"
         "--thin-reach true (with --reach <D>) thins the primers the CSV would get on that reach, after everything\n"
         "else: --existing-primers stay, then the primer reaching the most columns nothing kept reaches yet is kept\n"
         "until none reaches --thin-reach-min-gain <N> (default 1) new columns. No reached column is lost at N = 1.\n"
         "The report and --reach-out then describe the kept primers.\n";
    return u;
}

Args Args::parse(int argc, const char *const *argv)
{
    Args a;
    for (const auto &o : kOpts)   // environment first, the command line overrides it (clap)
        if (const char *e = std::getenv(o.env))
            if (*e) assign(a, o, e);
    for (int i = 1; i < argc; ++i) {
        std::string tok = argv[i], val;
        bool has_val = false;
        const size_t eq = tok.find('=');
        if (tok.rfind("--", 0) == 0 && eq != std::string::npos) {
            val = tok.substr(eq + 1);
            tok = tok.substr(0, eq);
            has_val = true;
        }
        auto need = [&]() -> std::string {
            if (has_val) return val;
            if (i + 1 >= argc)
                throw UsageError("error: a value is required for '" + tok + " <...>' but none was supplied");
            return argv[++i];
        };
        if (tok == "-h" || tok == "--help") throw UsageError(usage());
        if (tok == "-i" || tok == "--input") { a.input = need(); continue; }
        if (tok == "-o" || tok == "--output") { a.output = need(); continue; }
        if (tok == "--stddev-population") { a.stddev_population = true; continue; }
        bool found = false;
        for (const auto &o : kOpts)
            if (tok == o.flag) {
                assign(a, o, need());
                found = true;
                break;
            }
        if (!found) throw UsageError("error: unexpected argument '" + tok + "' found\n\n" + usage());
    }
    if (a.input.empty() || a.output.empty())
        throw UsageError("error: the following required arguments were not provided:\n"
                         "  --input <INPUT>\n  --output <OUTPUT>\n\n" + usage());
    if (a.tubes > 64)
        throw UsageError("error: invalid value '" + std::to_string(a.tubes) + "' for '--tubes <...>'\n  [0 .. 64]");
    if (a.tubes > 0) {   // one device, one call, and a panel's own tubes are unknown
        if (!a.devices.empty())
            throw UsageError("error: '--tubes' runs on one device and cannot be combined with '--devices'");
        if (a.cover_on_device == "true")
            throw UsageError("error: '--tubes' replaces the vertex cover and cannot be combined with "
                             "'--cover-on-device true'");
        if (!a.existing_primers.empty())
            throw UsageError("error: '--tubes' cannot be combined with '--existing-primers': the tubes of the panel's "
                             "primers are unknown");
    }
    if (a.repick_rounds > 16)
        throw UsageError("error: invalid value '" + std::to_string(a.repick_rounds) +
                         "' for '--repick-rounds <...>'\n  [0 .. 16]");
    if (a.repick_rounds > 0) {   // every round is a one-device panel extension, and a panel's tubes are unknown
        if (a.tubes > 0)
            throw UsageError("error: '--repick-rounds' cannot be combined with '--tubes': a later round extends the "
                             "earlier rounds' primers, whose tubes it cannot change");
        if (!a.devices.empty())
            throw UsageError("error: '--repick-rounds' runs on one device and cannot be combined with '--devices'");
    }
    if (a.coverage_mismatches > a.kmer_size)
        throw UsageError("error: '--coverage-mismatches " + std::to_string(a.coverage_mismatches) +
                         "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
    if (!a.coverage_tm_text.empty()) {
        char *end = nullptr;
        a.coverage_tm = std::strtof(a.coverage_tm_text.c_str(), &end);
        if (*end || std::isnan(a.coverage_tm))
            throw UsageError("error: invalid value '" + a.coverage_tm_text + "' for '--coverage-tm'");
        if (!a.devices.empty())
            throw UsageError("error: '--coverage-tm' runs on one device and cannot be combined with '--devices'");
        if (a.kmer_size < 2)
            throw UsageError("error: '--coverage-tm' needs '--kmer-size' of at least 2");
        a.coverage_scored = true;
        if (a.coverage_thal.empty()) a.coverage_thal = "any";
        if (a.coverage_thal != "any" && a.coverage_thal != "end1")
            throw UsageError("error: invalid value '" + a.coverage_thal +
                             "' for '--coverage-thal <...>'\n  [possible values: any, end1]");
    }
    if (!a.max_cross_dimer_end_tm_text.empty()) {
        char *end = nullptr;
        a.max_cross_dimer_end_tm = std::strtof(a.max_cross_dimer_end_tm_text.c_str(), &end);
        if (*end || std::isnan(a.max_cross_dimer_end_tm))
            throw UsageError("error: invalid value '" + a.max_cross_dimer_end_tm_text + "' for '--max-cross-dimer-end-tm'");
        if (a.kmer_size < 2) throw UsageError("error: '--max-cross-dimer-end-tm' needs '--kmer-size' of at least 2");
        a.cross_dimer_end = true;
    }
    if (a.coverage_mismatches > 0 || a.coverage_scored) {
        const std::string &v = a.coverage_3p_exact_text;
        char *end = nullptr;
        const long e = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || e < 0) throw UsageError("error: invalid value '" + v + "' for '--coverage-3p-exact'");
        if (e > a.kmer_size)
            throw UsageError("error: '--coverage-3p-exact " + v + "' is larger than '--kmer-size " +
                             std::to_string(a.kmer_size) + "'");
        a.coverage_3p_exact = (int)e;
    }
    if (a.select_by_coverage == "true") {
        if (a.select_depth < 1 || a.select_depth > 255)
            throw UsageError("error: invalid value '" + std::to_string(a.select_depth) +
                             "' for '--select-depth <...>'\n  [1 .. 255]");
        if (a.thin_panel == "true")
            throw UsageError("error: '--select-by-coverage true' keeps only what the coverage needs and cannot be "
                             "combined with '--thin-panel true'");
        if (a.keep_all == "true")
            throw UsageError("error: '--select-by-coverage true' drops primers and cannot be combined with "
                             "'--keep-all true'");
        if (!a.devices.empty())
            throw UsageError("error: '--select-by-coverage true' runs on one device and cannot be combined with "
                             "'--devices'");
        if (a.cover_on_device == "true")
            throw UsageError("error: '--select-by-coverage true' replaces the vertex cover and cannot be combined with "
                             "'--cover-on-device true'");
    }
    if (a.thin_panel == "true" || a.select_by_coverage == "true") {
        if (a.thin_panel == "true" && a.keep_all == "true")
            throw UsageError("error: '--thin-panel true' drops primers and cannot be combined with '--keep-all true'");
        if (a.thin_panel == "true" && !a.devices.empty())
            throw UsageError("error: '--thin-panel true' runs on one device and cannot be combined with '--devices'");
        if (a.thin_mismatches > a.kmer_size)
            throw UsageError("error: '--thin-mismatches " + std::to_string(a.thin_mismatches) +
                             "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
        const std::string &v = a.thin_3p_exact_text;
        char *end = nullptr;
        const long e = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || e < 0) throw UsageError("error: invalid value '" + v + "' for '--thin-3p-exact'");
        if (e > a.kmer_size)
            throw UsageError("error: '--thin-3p-exact " + v + "' is larger than '--kmer-size " +
                             std::to_string(a.kmer_size) + "'");
        a.thin_3p_exact = (int)e;
        if (a.thin_min_gain < 1)
            throw UsageError("error: invalid value '" + std::to_string(a.thin_min_gain) +
                             "' for '--thin-min-gain <...>'\n  [1 ..]");
        if (a.thin_panel == "true") {   // the selection's depth is --select-depth
            if (a.thin_depth < 1 || a.thin_depth > 255)
                throw UsageError("error: invalid value '" + std::to_string(a.thin_depth) +
                                 "' for '--thin-depth <...>'\n  [1 .. 255]");
        } else if (a.thin_depth > 1) {
            throw UsageError("error: '--thin-depth " + std::to_string(a.thin_depth) +
                             "' cannot be combined with '--select-by-coverage true': the selection's depth is "
                             "'--select-depth <R>'");
        }
        if (!a.thin_tm_text.empty()) {
            a.thin_tm = std::strtof(a.thin_tm_text.c_str(), &end);
            if (*end || std::isnan(a.thin_tm))
                throw UsageError("error: invalid value '" + a.thin_tm_text + "' for '--thin-tm'");
            if (a.kmer_size < 2) throw UsageError("error: '--thin-tm' needs '--kmer-size' of at least 2");
            a.thin_scored = true;
            if (a.thin_thal.empty()) a.thin_thal = "any";
            if (a.thin_thal != "any" && a.thin_thal != "end1")
                throw UsageError("error: invalid value '" + a.thin_thal +
                                 "' for '--thin-thal <...>'\n  [possible values: any, end1]");
        }
    }
    if (!a.genome_weights.empty()) {
        const bool thin = a.thin_panel == "true", select = a.select_by_coverage == "true";
        if (!thin && !select)
            throw UsageError("error: '--genome-weights' weighs the segments of '--thin-panel true' or "
                             "'--select-by-coverage true' and does nothing without one of them");
        if ((thin && a.thin_depth > 1) || (select && a.select_depth > 1))
            throw UsageError(std::string("error: '--genome-weights' with '") + (thin ? "--thin-depth" : "--select-depth") +
                             "' above 1 is not built yet: weights run at depth 1");
        if (thin && a.thin_scored)
            throw UsageError("error: '--genome-weights' with '--thin-panel true --thin-tm' is not built yet: the "
                             "weighted thinning runs on the string rule");
    }
    for (const auto &given : {std::make_pair("--default-primer-cost", &a.default_primer_cost_text),
                              std::make_pair("--background-site-cost", &a.background_site_cost_text)}) {
        const std::string &v = *given.second;   // an integer 1 .. 2^32 - 1
        if (v.empty()) continue;
        char *end = nullptr;
        errno = 0;
        const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
        if (v.find_first_not_of("0123456789") != std::string::npos || *end || errno || x < 1 || x > 0xFFFFFFFFull)
            throw UsageError(std::string("error: invalid value '") + v + "' for '" + given.first +
                             " <...>'\n  [1 .. 4294967295]");
        (given.second == &a.default_primer_cost_text ? a.default_primer_cost : a.background_site_cost) = (uint32_t)x;
    }
    if (!a.primer_costs.empty() || a.background_site_cost) {
        const bool thin = a.thin_panel == "true", select = a.select_by_coverage == "true";
        const char *both = "'--primer-costs' and '--background-site-cost'";
        if (!a.devices.empty())   // first: the two switches refuse '--devices' themselves
            throw UsageError(std::string("error: ") + both + " run on one device and cannot be combined with "
                             "'--devices'");
        if (!thin && !select)
            throw UsageError(std::string("error: ") + both + " price the primers of '--thin-panel true' or "
                             "'--select-by-coverage true' and do nothing without one of them");
        if (a.background_site_cost && a.background.empty())
            throw UsageError("error: '--background-site-cost' needs '--background <FASTA>'");
        if ((thin && a.thin_depth > 1) || (select && a.select_depth > 1))
            throw UsageError(std::string("error: ") + both + " with '" + (thin ? "--thin-depth" : "--select-depth") +
                             "' above 1 are not built yet: costs run at depth 1");
        if (thin && a.thin_scored)
            throw UsageError(std::string("error: ") + both + " with '--thin-panel true --thin-tm' are not built yet: "
                             "the held thinning has no cost form");
        a.primer_costs_on = true;
    }
    if (a.seed_mismatches >= 0 || !a.seed_tm_text.empty() || !a.seed_thal.empty() || !a.seed_3p_exact_text.empty()) {
        if (!a.devices.empty())
            throw UsageError("error: '--seed-mismatches', '--seed-3p-exact', '--seed-tm' and '--seed-thal' run on one "
                             "device and cannot be combined with '--devices'");
        if (!a.seed_thal.empty() && a.seed_tm_text.empty())
            throw UsageError("error: '--seed-thal' needs '--seed-tm <C>'");
    }
    // read only when a round can seed, as the --thin-* values are read only with their switch
    if ((!a.existing_primers.empty() || a.repick_rounds > 0) && (a.seed_mismatches >= 0 || !a.seed_tm_text.empty())) {
        char *end = nullptr;
        if (!a.seed_tm_text.empty()) {
            a.seed_tm = std::strtof(a.seed_tm_text.c_str(), &end);
            if (*end || std::isnan(a.seed_tm))
                throw UsageError("error: invalid value '" + a.seed_tm_text + "' for '--seed-tm'");
            if (a.kmer_size < 2) throw UsageError("error: '--seed-tm' needs '--kmer-size' of at least 2");
            a.seed_scored = true;
            if (a.seed_thal.empty()) a.seed_thal = "any";
            if (a.seed_thal != "any" && a.seed_thal != "end1")
                throw UsageError("error: invalid value '" + a.seed_thal +
                                 "' for '--seed-thal <...>'\n  [possible values: any, end1]");
            if (a.seed_mismatches < 0) a.seed_mismatches = 0;
        }
        if (a.seed_mismatches > a.kmer_size)
            throw UsageError("error: '--seed-mismatches " + std::to_string(a.seed_mismatches) +
                             "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
        const std::string v = a.seed_3p_exact_text.empty() ? "3" : a.seed_3p_exact_text;
        const long e = std::strtol(v.c_str(), &end, 10);
        if (*end || e < 0) throw UsageError("error: invalid value '" + v + "' for '--seed-3p-exact'");
        if (e > a.kmer_size)
            throw UsageError("error: '--seed-3p-exact " + v + "' is larger than '--kmer-size " +
                             std::to_string(a.kmer_size) + "'");
        a.seed_3p_exact = (int)e;
        a.seed_tolerant = true;
    }
    if (a.background.empty()) {
        for (const auto &given : {std::make_pair("--background-mismatches", a.background_mismatches),
                                  std::make_pair("--background-3p-exact", a.background_3p_exact),
                                  std::make_pair("--max-background-sites", a.max_background_sites)})
            if (given.second >= 0)
                throw UsageError(std::string("error: '") + given.first + "' needs '--background <FASTA>'");
        for (const auto &given : {std::make_pair("--background-tm", &a.background_tm_text),
                                  std::make_pair("--background-thal", &a.background_thal)})
            if (!given.second->empty())
                throw UsageError(std::string("error: '") + given.first + "' needs '--background <FASTA>'");
    }
    if (!a.background_tm_text.empty()) {
        char *end = nullptr;
        a.background_tm = std::strtof(a.background_tm_text.c_str(), &end);
        if (*end || std::isnan(a.background_tm))
            throw UsageError("error: invalid value '" + a.background_tm_text + "' for '--background-tm'");
        a.background_scored = true;
    }
    for (const auto &given : {std::make_pair("--background-amplicon-max", a.background_amplicon_max),
                              std::make_pair("--background-amplicon-min", a.background_amplicon_min)}) {
        if (given.second < 0) continue;
        if (a.background.empty())
            throw UsageError(std::string("error: '") + given.first + "' needs '--background <FASTA>'");
        if (!a.background_scored)
            throw UsageError(std::string("error: '") + given.first + "' needs '--background-tm <C>'");
    }
    if (a.background_flank >= 0) {
        if (a.background.empty()) throw UsageError("error: '--background-flank' needs '--background <FASTA>'");
        if (!a.background_scored) throw UsageError("error: '--background-flank' needs '--background-tm <C>'");
        if (a.background_flank > 4)
            throw UsageError("error: invalid value '" + std::to_string(a.background_flank) +
                             "' for '--background-flank <...>'\n  [possible values: 0, 1, 2, 3, 4]");
        if (a.kmer_size + 2 * a.background_flank > 32)
            throw UsageError("error: '--kmer-size " + std::to_string(a.kmer_size) + "' with '--background-flank " +
                             std::to_string(a.background_flank) + "' is longer than 32 bases");
    } else {
        a.background_flank = 0;
    }
    if (a.background_amplicon_min >= 0 && a.background_amplicon_max < 0)
        throw UsageError("error: '--background-amplicon-min' needs '--background-amplicon-max <LEN>'");
    if (a.background_amplicon_max >= 0) {
        if (a.background_amplicon_min < 0) a.background_amplicon_min = a.kmer_size;
        if (a.background_amplicon_min < a.kmer_size)
            throw UsageError("error: '--background-amplicon-min " + std::to_string(a.background_amplicon_min) +
                             "' is smaller than '--kmer-size " + std::to_string(a.kmer_size) + "'");
        if (a.background_amplicon_min > a.background_amplicon_max)
            throw UsageError("error: '--background-amplicon-min " + std::to_string(a.background_amplicon_min) +
                             "' is larger than '--background-amplicon-max " +
                             std::to_string(a.background_amplicon_max) + "'");
    }
    if (a.background_thal.empty()) a.background_thal = "any";
    if (a.background_thal != "any" && a.background_thal != "end1")
        throw UsageError("error: invalid value '" + a.background_thal +
                         "' for '--background-thal <...>'\n  [possible values: any, end1]");
    if (a.background_mismatches > a.kmer_size)
        throw UsageError("error: '--background-mismatches " + std::to_string(a.background_mismatches) +
                         "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
    if (a.background_3p_exact > a.kmer_size)
        throw UsageError("error: '--background-3p-exact " + std::to_string(a.background_3p_exact) +
                         "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
    if (a.background_mismatches < 0) a.background_mismatches = std::min(2, a.kmer_size);
    if (a.background_3p_exact < 0) a.background_3p_exact = std::min(3, a.kmer_size);
    if (a.thin_reach_min_gain < 1)
        throw UsageError("error: invalid value '" + std::to_string(a.thin_reach_min_gain) +
                         "' for '--thin-reach-min-gain <...>'\n  [1 ..]");
    if (a.reach_text.empty() && a.thin_reach == "true") throw UsageError("error: '--thin-reach' needs '--reach <D>'");
    if (a.thin_reach != "true" && a.thin_reach_min_gain != 1)
        throw UsageError("error: '--thin-reach-min-gain' needs '--thin-reach true'");
    if (a.reach_text.empty()) {
        for (const auto &given : {std::make_pair("--reach-mismatches", a.reach_mismatches),
                                  std::make_pair("--reach-3p-exact", a.reach_3p_exact)})
            if (given.second >= 0) throw UsageError(std::string("error: '") + given.first + "' needs '--reach <D>'");
        for (const auto &given : {std::make_pair("--reach-tm", &a.reach_tm_text),
                                  std::make_pair("--reach-thal", &a.reach_thal),
                                  std::make_pair("--reach-out", &a.reach_out)})
            if (!given.second->empty())
                throw UsageError(std::string("error: '") + given.first + "' needs '--reach <D>'");
    } else {
        char *end = nullptr;
        const unsigned long long d = std::strtoull(a.reach_text.c_str(), &end, 10);
        if (*end || a.reach_text[0] == '-' || a.reach_text[0] == '+' || d >= (1ull << 31))
            throw UsageError("error: invalid value '" + a.reach_text + "' for '--reach <D>'\n  [possible values: "
                             "the k-mer size .. 2147483647]");
        if (a.kmer_size < 2) throw UsageError("error: '--reach' needs '--kmer-size' of at least 2");
        if (d < (unsigned long long)a.kmer_size)
            throw UsageError("error: '--reach " + a.reach_text + "' is smaller than '--kmer-size " +
                             std::to_string(a.kmer_size) + "'");
        a.reach = (long long)d;
        if (!a.reach_thal.empty() && a.reach_tm_text.empty())
            throw UsageError("error: '--reach-thal' needs '--reach-tm <C>'");
        if (!a.reach_tm_text.empty()) {
            a.reach_tm = std::strtof(a.reach_tm_text.c_str(), &end);
            if (*end || std::isnan(a.reach_tm))
                throw UsageError("error: invalid value '" + a.reach_tm_text + "' for '--reach-tm'");
            a.reach_scored = true;
            if (a.reach_thal.empty()) a.reach_thal = "any";
            if (a.reach_thal != "any" && a.reach_thal != "end1")
                throw UsageError("error: invalid value '" + a.reach_thal +
                                 "' for '--reach-thal <...>'\n  [possible values: any, end1]");
        }
        if (a.reach_mismatches > a.kmer_size)
            throw UsageError("error: '--reach-mismatches " + std::to_string(a.reach_mismatches) +
                             "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
        if (a.reach_3p_exact > a.kmer_size)
            throw UsageError("error: '--reach-3p-exact " + std::to_string(a.reach_3p_exact) +
                             "' is larger than '--kmer-size " + std::to_string(a.kmer_size) + "'");
        if (a.reach_mismatches < 0) a.reach_mismatches = std::min(2, a.kmer_size);
        if (a.reach_3p_exact < 0) a.reach_3p_exact = std::min(3, a.kmer_size);
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
// FASTA (main.rs:108-122; seq_io semantics: id = header up to the first space, lines joined)
// ---------------------------------------------------------------------------------------------
namespace {

// records of the byte range [p, end): one pass; sequence bytes go through a 256-entry table
// (upper case, U -> T).  Bytes before the first header of the range are ignored.
std::vector<SequenceRecord> parse_fasta_range(const char *p, const char *end)
{
    static const auto table = [] {
        std::array<char, 256> t{};
        for (int c = 0; c < 256; ++c) {
            char u = (char)std::toupper(c);
            t[(size_t)c] = u == 'U' ? 'T' : u;
        }
        return t;
    }();
    std::vector<SequenceRecord> out;
    size_t reserve_hint = 0;
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
        const char *stop = nl ? nl : end;
        const char *last = stop;
        if (last > p && last[-1] == '\r') --last;
        if (last > p && *p == '>') {
            if (!out.empty()) reserve_hint = std::max(reserve_hint, out.back().sequence.size());
            const char *sp = static_cast<const char *>(std::memchr(p, ' ', (size_t)(last - p)));
            out.push_back({std::string(p + 1, sp ? sp : last), std::string()});
            out.back().sequence.reserve(reserve_hint);
        } else if (!out.empty()) {
            std::string &seq = out.back().sequence;
            const size_t at = seq.size();
            seq.resize(at + (size_t)(last - p));
            for (size_t q = 0; q < (size_t)(last - p); ++q) seq[at + q] = table[(unsigned char)p[q]];
        }
        p = nl ? nl + 1 : end;
    }
    return out;
}

}  // namespace

std::vector<SequenceRecord> to_records(const std::string &fasta)
{
    return to_records(fasta.data(), fasta.size());
}

std::vector<SequenceRecord> to_records(const char *base, size_t size)
{
    const char *end = base + size;
    // large inputs: cut at header lines and parse the pieces on the host's cores
    const size_t n_threads = std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), 16,
                                               size / (8u << 20)});
    if (n_threads < 2) return parse_fasta_range(base, end);
    std::vector<const char *> cut{base};
    for (size_t t = 1; t < n_threads; ++t) {
        const char *p = base + size / n_threads * t;
        const char *hit = nullptr;
        while (p < end) {   // next line that starts with '>'
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            if (!nl || nl + 1 >= end) break;
            if (nl[1] == '>') {
                hit = nl + 1;
                break;
            }
            p = nl + 1;
        }
        if (hit && hit > cut.back()) cut.push_back(hit);
    }
    cut.push_back(end);
    std::vector<std::vector<SequenceRecord>> parts(cut.size() - 1);
    std::vector<std::thread> pool;
    for (size_t t = 0; t + 1 < cut.size(); ++t)
        pool.emplace_back([&, t] { parts[t] = parse_fasta_range(cut[t], cut[t + 1]); });
    for (auto &th : pool) th.join();
    std::vector<SequenceRecord> out;
    size_t total = 0;
    for (const auto &v : parts) total += v.size();
    out.reserve(total);
    for (auto &v : parts)
        for (auto &r : v) out.push_back(std::move(r));
    return out;
}

std::string reverse_complement(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) switch (c) {
        case 'A': c = 'T'; break;
        case 'T': c = 'A'; break;
        case 'U': c = 'A'; break;
        case 'C': c = 'G'; break;
        case 'G': c = 'C'; break;
        default: break;
        }
    return r;
}

// ---------------------------------------------------------------------------------------------
// engine handle
// ---------------------------------------------------------------------------------------------
Engine::Engine(int device, const std::string &params_path)
{
    const int rc = msspe_create(device, params_path.empty() ? nullptr : params_path.c_str(), &ctx_);
    if (rc) {
        const std::string msg = ctx_ ? msspe_last_error(ctx_) : "allocation failed";
        if (ctx_) msspe_destroy(ctx_);
        ctx_ = nullptr;
        throw std::runtime_error("msspe_create: " + msg);
    }
}
Engine::Engine(const std::vector<int> &devices, const std::string &params_path)
{
    const int rc = msspe_group_create(devices.data(), (int)devices.size(), params_path.empty() ? nullptr : params_path.c_str(),
                                      nullptr, &group_);
    if (rc) {
        const std::string msg = group_ ? msspe_group_last_error(group_) : "allocation failed";
        if (group_) msspe_group_destroy(group_);
        group_ = nullptr;
        throw std::runtime_error("msspe_group_create: " + msg);
    }
    ctx_ = msspe_group_member(group_, 0);
}
Engine::~Engine()
{
    if (group_) msspe_group_destroy(group_);   // owns its members
    else if (ctx_) msspe_destroy(ctx_);
}
void Engine::fail_group(int rc) const
{
    throw std::runtime_error(std::string("libmsspe_hip status ") + std::to_string(rc) + ": " + msspe_group_last_error(group_));
}
void Engine::fail(int rc) const
{
    throw std::runtime_error(std::string("libmsspe_hip status ") + std::to_string(rc) + ": " +
                             msspe_last_error(ctx_));
}

// ---------------------------------------------------------------------------------------------
// stage A (main.rs:196-235, 331-406)
// ---------------------------------------------------------------------------------------------
DeviceAlignment::DeviceAlignment(Engine &eng, const std::vector<SequenceRecord> &records) : eng_(eng)
{
    // The device path takes one rectangular byte matrix.  Rows shorter than the longest are
    // padded with '-': partition j starts at the same column in every row (main.rs:173-181), pad
    // columns invalidate every k-mer that touches them (main.rs:167), so the extra all-pad
    // partitions of a short row hold no k-mers and can neither be counted nor covered -- the
    // winners are exactly those of the reference's per-record partitioning.
    for (const auto &r : records) len_ = std::max(len_, r.sequence.size());
    rows_ = (int)records.size();
    // rows go to the device through the library's pinned staging; no rectangular host copy
    std::vector<const char *> rows(records.size());
    std::vector<size_t> bytes(records.size());
    for (size_t r = 0; r < records.size(); ++r) {
        rows[r] = records[r].sequence.data();
        bytes[r] = records[r].sequence.size();
    }
    // packed on the device: 2-bit bases + validity bit (3/8 byte per column stay resident)
    const int rc = msspe_device_put_rows_packed(eng.ctx(), rows.data(), bytes.data(), rows_, len_, &dev_);
    if (rc) eng.fail(rc);
}

DeviceAlignment::~DeviceAlignment()
{
    if (dev_) (void)msspe_device_free(eng_.ctx(), dev_);
}

std::vector<KmerFrequency> find_candidates_kmers(Engine &eng, const DeviceAlignment &aln, uint8_t direction,
                                                 const ProgramConfig &cfg, int segment_size,
                                                 int overlap_size, int window_size)
{
    if (overlap_size < window_size)   // main.rs:201-203
        throw Panic("Overlap windows size must be greater or equal than search windows size");
    std::vector<KmerFrequency> out;
    if (aln.rows() == 0) return out;
    msspe_kmer_opt opt{segment_size, overlap_size, window_size, cfg.primer_config.kmer_size,
                       cfg.max_iterations, cfg.max_mismatch_segments};
    const int cap = std::max(1, cfg.max_iterations);
    std::vector<uint64_t> words((size_t)cap);
    std::vector<uint32_t> freq((size_t)cap);
    int n = 0;
    const int rc = msspe_kmer_candidates_packed_dev(eng.ctx(), aln.device(), aln.rows(), aln.length(), &opt, direction,
                                             words.data(), freq.data(), cap, &n);
    if (rc) eng.fail(rc);
    std::vector<char> buf((size_t)opt.kmer_size + 1);
    for (int i = 0; i < n; ++i) {
        msspe_unpack_oligo(words[(size_t)i], opt.kmer_size, buf.data());
        out.push_back({std::string(buf.data()), direction, freq[(size_t)i]});
    }
    return out;
}

// Both directions in one engine call (msspe_kmer_candidates_both_packed_dev: two streams, two host threads); what the
// reference gets from its two find_candidates_kmers calls, main.rs:673-690.
std::pair<std::vector<KmerFrequency>, std::vector<KmerFrequency>> find_candidates_kmers_both(
    Engine &eng, const DeviceAlignment &aln, const ProgramConfig &cfg, int segment_size, int overlap_size, int window_size,
    const std::vector<std::string> &seed_f, const std::vector<std::string> &seed_r,
    const std::vector<std::string> &excl_f, const std::vector<std::string> &excl_r, const msspe_seed_rule *rule,
    size_t *seed_covered)
{
    if (overlap_size < window_size)   // main.rs:201-203
        throw Panic("Overlap windows size must be greater or equal than search windows size");
    std::pair<std::vector<KmerFrequency>, std::vector<KmerFrequency>> out;
    if (seed_covered) seed_covered[0] = seed_covered[1] = 0;
    if (aln.rows() == 0) return out;
    msspe_kmer_opt opt{segment_size, overlap_size, window_size, cfg.primer_config.kmer_size,
                       cfg.max_iterations, cfg.max_mismatch_segments};
    const int cap = std::max(1, cfg.max_iterations);
    std::vector<uint64_t> words[2] = {std::vector<uint64_t>((size_t)cap), std::vector<uint64_t>((size_t)cap)};
    std::vector<uint32_t> freq[2] = {std::vector<uint32_t>((size_t)cap), std::vector<uint32_t>((size_t)cap)};
    int n[2] = {0, 0};
    int rc;
    auto pack = [&](const std::vector<std::string> &list) {
        std::string flat;
        for (const auto &w : list) flat += w;
        std::vector<uint64_t> packed(list.size() + 1);
        if (!list.empty() && (rc = msspe_pack_oligos(flat.data(), (int)list.size(), opt.kmer_size, packed.data())))
            eng.fail(rc);
        return packed;
    };
    if (rule) {   // the seeds cover what they match under the rule; the state before the first iteration comes back
        const std::vector<uint64_t> sf = pack(seed_f), sr = pack(seed_r), xf = pack(excl_f), xr = pack(excl_r);
        const msspe_kmer_sets fwd = {sf.data(), (int)seed_f.size(), xf.data(), (int)excl_f.size()};
        const msspe_kmer_sets rev = {sr.data(), (int)seed_r.size(), xr.data(), (int)excl_r.size()};
        const size_t L = aln.length();
        const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
        std::vector<uint8_t> cov[2] = {std::vector<uint8_t>(P * (size_t)aln.rows() + 1),
                                       std::vector<uint8_t>(P * (size_t)aln.rows() + 1)};
        rc = msspe_kmer_candidates_both_tolerant_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &fwd, &rev, rule,
                                                            words[0].data(), freq[0].data(), &n[0], words[1].data(),
                                                            freq[1].data(), &n[1], cap, cov[0].data(), nullptr,
                                                            cov[1].data(), nullptr);
        if (!rc && seed_covered)
            for (int d = 0; d < 2; ++d)
                seed_covered[d] = (size_t)std::count(cov[d].begin(), cov[d].end() - 1, (uint8_t)1);
    } else if (!excl_f.empty() || !excl_r.empty()) {
        const std::vector<uint64_t> sf = pack(seed_f), sr = pack(seed_r), xf = pack(excl_f), xr = pack(excl_r);
        const msspe_kmer_sets fwd = {sf.data(), (int)seed_f.size(), xf.data(), (int)excl_f.size()};
        const msspe_kmer_sets rev = {sr.data(), (int)seed_r.size(), xr.data(), (int)excl_r.size()};
        rc = msspe_kmer_candidates_both_sets_packed_dev(eng.ctx(), aln.device(), aln.rows(), aln.length(), &opt, &fwd,
                                                        &rev, words[0].data(), freq[0].data(), &n[0], words[1].data(),
                                                        freq[1].data(), &n[1], cap);
    } else if (seed_f.empty() && seed_r.empty()) {
        rc = msspe_kmer_candidates_both_packed_dev(eng.ctx(), aln.device(), aln.rows(), aln.length(), &opt,
                                                   words[0].data(), freq[0].data(), &n[0], words[1].data(),
                                                   freq[1].data(), &n[1], cap);
    } else {
        std::vector<uint64_t> sw[2];
        for (int d = 0; d < 2; ++d) {
            const auto &seed = d ? seed_r : seed_f;
            std::string flat;
            for (const auto &w : seed) flat += w;
            sw[d].resize(seed.size() + 1);
            if (!seed.empty() && (rc = msspe_pack_oligos(flat.data(), (int)seed.size(), opt.kmer_size, sw[d].data())))
                eng.fail(rc);
        }
        rc = msspe_kmer_candidates_both_seeded_packed_dev(eng.ctx(), aln.device(), aln.rows(), aln.length(), &opt,
                                                          sw[0].data(), (int)seed_f.size(), sw[1].data(),
                                                          (int)seed_r.size(), words[0].data(), freq[0].data(), &n[0],
                                                          words[1].data(), freq[1].data(), &n[1], cap);
    }
    if (rc) eng.fail(rc);
    std::vector<char> buf((size_t)opt.kmer_size + 1);
    for (int d = 0; d < 2; ++d) {
        auto &dst = d ? out.second : out.first;
        for (int i = 0; i < n[d]; ++i) {
            msspe_unpack_oligo(words[d][(size_t)i], opt.kmer_size, buf.data());
            dst.push_back({std::string(buf.data()), (uint8_t)(d ? SEQ_DIR_REV : SEQ_DIR_FWD), freq[d][(size_t)i]});
        }
    }
    return out;
}

std::vector<KmerFrequency> find_candidates_kmers(Engine &eng, const std::vector<SequenceRecord> &records,
                                                 uint8_t direction, const ProgramConfig &cfg,
                                                 int segment_size, int overlap_size, int window_size)
{
    if (overlap_size < window_size)   // main.rs:201-203
        throw Panic("Overlap windows size must be greater or equal than search windows size");
    if (records.empty()) return {};
    const DeviceAlignment aln(eng, records);
    return find_candidates_kmers(eng, aln, direction, cfg, segment_size, overlap_size, window_size);
}

// ---------------------------------------------------------------------------------------------
// stage B (primer.rs:143-166; main.rs:408-516)
// ---------------------------------------------------------------------------------------------
std::vector<PrimerInfo> check_primers(Engine &eng, const std::vector<std::string> &primers)
{
    std::vector<PrimerInfo> out;
    if (primers.empty()) return out;
    const int n = (int)primers.size(), k = (int)primers[0].size();
    std::string flat;
    for (const auto &p : primers) {
        if ((int)p.size() != k) throw std::runtime_error("primers of unequal length");
        flat += p;
    }
    std::vector<double> tm((size_t)n), gc((size_t)n), any((size_t)n), end((size_t)n), hp((size_t)n);
    msspe_chem chem;
    msspe_chem_primer3_defaults(&chem);   // primer.rs:125-140 sends only size / Tm bounds
    if (eng.group()) {   // oligos are independent: a slice per device
        const int rc = msspe_oligo_stats_group(eng.group(), flat.data(), n, k, &chem, tm.data(), gc.data(), any.data(),
                                               end.data(), hp.data());
        if (rc) eng.fail_group(rc);
    } else {
        const int rc = msspe_oligo_stats(eng.ctx(), flat.data(), n, k, &chem, tm.data(), gc.data(),
                                         any.data(), end.data(), hp.data());
        if (rc) eng.fail(rc);
    }
    for (int i = 0; i < n; ++i) {
        PrimerInfo p;
        p.id = primers[(size_t)i];
        p.tm = msspe_round_fixed_f32(tm[(size_t)i], 3);            // PRIMER_LEFT_0_TM=%.3f -> f32
        p.gc = msspe_round_fixed_f32(gc[(size_t)i], 3);
        p.self_any_th = msspe_round_fixed_f32(any[(size_t)i], 2);  // ..._TH=%.2f -> f32
        p.self_end_th = msspe_round_fixed_f32(end[(size_t)i], 2);
        p.hairpin_th = msspe_round_fixed_f32(hp[(size_t)i], 2);
        out.push_back(p);
    }
    return out;
}

void get_tm_stat(const std::vector<PrimerInfo> &info, bool population, float &mean, float &std)
{
    float sum = 0.0f;
    for (const auto &p : info) sum += p.tm;   // main.rs:464: sequential f32 sum
    mean = sum / (float)info.size();
    float acc = 0.0f;
    for (const auto &p : info) {
        const float d = p.tm - mean;
        acc += d * d;
    }
    const float div = population ? (float)info.size() : (float)(info.size() - 1);
    std = info.size() > (population ? 0u : 1u) ? std::sqrt(acc / div) : 0.0f;
}

bool tm_in_threshold(float tm, float mean, float std, float diff)
{
    return std::fabs(tm - mean) <= (diff * std);
}

bool is_run(const std::string &kmer)   // main.rs:478-490: only the trailing run counts
{
    int runs = 0;
    char last = ' ';
    for (char c : kmer) {
        if (c == last) runs += 1;
        else runs = 0;
        last = c;
    }
    return runs >= 5;
}

std::vector<KmerStat> get_kmer_stats(Engine &eng, const std::vector<KmerFrequency> &kmers,
                                     const ProgramConfig &cfg)
{
    std::vector<KmerStat> out;
    if (kmers.empty()) return out;
    std::vector<std::string> primers;
    for (const auto &k : kmers) primers.push_back(k.word);
    const auto info = check_primers(eng, primers);
    std::map<std::string, const PrimerInfo *> by_id;
    for (const auto &p : info) by_id.emplace(p.id, &p);   // first entry wins (or_insert)
    float mean, std;
    get_tm_stat(info, cfg.stddev_population, mean, std);
    for (const auto &k : kmers) {
        const PrimerInfo *p = by_id.at(k.word);
        out.push_back({k.word, k.direction, p->gc, mean, std, p->tm,
                       tm_in_threshold(p->tm, mean, std, cfg.tm_stddev), p->self_any_th,
                       p->self_end_th, p->hairpin_th, is_run(k.word)});
    }
    return out;
}

std::vector<KmerStat> filter_kmers(const std::vector<KmerStat> &stats, const ProgramConfig &cfg)
{
    const PrimerConfig &pc = cfg.primer_config;
    std::vector<KmerStat> out;
    for (const auto &s : stats) {
        const bool pass_self_any = !cfg.check_self_dimers || (s.self_any_th < pc.max_self_dimer_any_tm);
        const bool pass_self_end = !cfg.check_self_dimers || (s.self_end_th < pc.max_self_dimer_end_tm);
        const bool pass_hairpin = !cfg.check_hairpin || (s.hairpin_th < pc.max_hairpin_tm);
        const bool pass_min_max = cfg.disable_min_max_tm || (s.tm > pc.min_tm && s.tm < pc.max_tm);
        const bool pass_stddev = cfg.disable_tm_stddev || s.tm_ok;
        if (pass_self_any && pass_self_end && pass_hairpin && pass_min_max && pass_stddev && !s.runs)
            out.push_back(s);
    }
    return out;
}

// ---------------------------------------------------------------------------------------------
// stage C (delta_g.rs:61-153) and the vertex cover (main.rs:754-798)
// ---------------------------------------------------------------------------------------------
// delta_g.rs:64-73: is the ordered pair (a, b) sent to ntthal at all?
bool ntthal_pair_sent(const std::string &a, const std::string &b, const ProgramConfig &cfg)
{
    if (!cfg.check_self_dimers && (a == b || reverse_complement(b) == a)) return false;
    return cfg.check_cross_dimers;
}

// delta_g.rs:61-81: every ordered pair that is sent, "a,b" per line, no trailing newline.  The engine
// takes the packed pool instead of this text; the function exists as the statement of WHICH pairs count
// (run_ntthal below applies the same predicate to the bitmap) and for the ntthal-compatible shim's tests.
std::string format_ntthal_input(const std::vector<std::string> &primers, const ProgramConfig &cfg)
{
    std::string out;
    for (const auto &a : primers)
        for (const auto &b : primers)
            if (ntthal_pair_sent(a, b, cfg)) out += a + "," + b + "\n";
    while (!out.empty() && (out.back() == '\n' || out.back() == ' ')) out.pop_back();   // .trim()
    return out;
}

namespace {
// the chemistry ntthal is called with: "{:.2}" strings of the f32 options (delta_g.rs:98-106)
msspe_chem ntthal_chem(const NtthalOptions &opts)
{
    auto two = [](float v) {
        char b[64];
        std::snprintf(b, sizeof b, "%.2f", (double)v);
        return std::strtod(b, nullptr);
    };
    return msspe_chem{two(opts.mv), two(opts.dv), two(opts.dntp), two(opts.conc), two(opts.t), 30};
}
// --max-cross-dimer-end-tm: the rule of every screen of the run
msspe_conflict_rule conflict_rule(const NtthalOptions &opts)
{
    return msspe_conflict_rule{1, opts.dg, 1, opts.end_tm};
}
// the line stdout gains: the ordered pairs of the n distinct oligos a screen under both rules saw, by kind
void note_kinds(const NtthalOptions &opts, size_t n, const uint64_t kinds[3])
{
    if (!opts.kinds_text) return;
    char b[256];
    std::snprintf(b, sizeof b, "Cross-dimer conflicts among %zu primers (dG < %.2f or 3'-end Tm >= %.2f): %llu dG only, "
                               "%llu 3'-end only, %llu both\n",
                  n, (double)opts.dg, (double)opts.end_tm, (unsigned long long)kinds[0], (unsigned long long)kinds[1],
                  (unsigned long long)kinds[2]);
    *opts.kinds_text += b;
}
// ... for the paths whose device call returns no counts: one more screen of the pool, counts only
void count_kinds(Engine &eng, const std::string &flat, int n, int k, const msspe_chem &chem, const NtthalOptions &opts)
{
    if (!opts.kinds_text) return;
    const msspe_conflict_rule rule = conflict_rule(opts);
    uint64_t kinds[3] = {0, 0, 0};
    const int rc = msspe_conflict_graph(eng.ctx(), flat.data(), n, k, &chem, &rule, nullptr, nullptr, kinds);
    if (rc) eng.fail(rc);
    note_kinds(opts, (size_t)n, kinds);
}
}  // namespace

ConflictGraph run_ntthal(Engine &eng, const std::vector<std::string> &primers,
                         const NtthalOptions &opts, const ProgramConfig &cfg)
{
    ConflictGraph g;
    // the reference's graph is keyed by the primer string: duplicates collapse into one node
    std::unordered_set<std::string> seen;
    for (const auto &p : primers)
        if (seen.insert(p).second) g.nodes.push_back(p);
    if (!cfg.check_cross_dimers || g.nodes.empty()) return g;   // delta_g.rs:71-73: no input at all
    const int n = (int)g.nodes.size(), k = (int)g.nodes[0].size();
    std::string flat;
    for (const auto &p : g.nodes) flat += p;
    const msspe_chem chem = ntthal_chem(opts);
    // the conflict edges as a list (about 0.5 % of the ordered pairs at the default threshold), not the
    // dense n x n bitmap; if the first guess is too small the call says how many there are
    std::vector<msspe_edge> edges((size_t)std::max<uint64_t>(4096, (uint64_t)n * (uint64_t)n / 64));
    uint64_t count = 0;
    // (with --devices: the rows of the pair matrix dealt out over the group, the same edges in the same order)
    auto screen = [&]() {
        return eng.group() ? msspe_cross_dimer_edges_group(eng.group(), flat.data(), n, k, &chem, opts.dg, edges.data(),
                                                           edges.size(), &count)
                           : msspe_cross_dimer_edges(eng.ctx(), flat.data(), n, k, &chem, opts.dg, edges.data(), edges.size(),
                                                     &count);
    };
    if (opts.use_end) {   // the union of the dG rule and the 3'-end rule, on member 0 where there is a group
        const msspe_conflict_rule rule = conflict_rule(opts);
        std::vector<msspe_kind_edge> kedges(edges.size());
        auto union_screen = [&]() {
            return msspe_conflict_graph_edges(eng.ctx(), flat.data(), n, k, &chem, &rule, kedges.data(), kedges.size(), &count);
        };
        int rc = union_screen();
        if (rc == MSSPE_ERR_CAPACITY) {
            kedges.resize((size_t)count);
            rc = union_screen();
        }
        if (rc) eng.fail(rc);
        uint64_t kinds[3] = {0, 0, 0};
        for (uint64_t e = 0; e < count; ++e) {
            const msspe_kind_edge &ed = kedges[(size_t)e];
            ++kinds[ed.kinds == MSSPE_KIND_ANY ? 0 : ed.kinds == MSSPE_KIND_END ? 1 : 2];
            const std::string &a = g.nodes[ed.a], &b = g.nodes[ed.b];
            if (!ntthal_pair_sent(a, b, cfg)) continue;
            g.edges[a].insert(b);
        }
        note_kinds(opts, (size_t)n, kinds);
        return g;
    }
    int rc = screen();
    if (rc == MSSPE_ERR_CAPACITY) {
        edges.resize((size_t)count);
        rc = screen();
    }
    if (rc) eng.group() ? eng.fail_group(rc) : eng.fail(rc);
    for (uint64_t e = 0; e < count; ++e) {
        const std::string &a = g.nodes[edges[(size_t)e].a], &b = g.nodes[edges[(size_t)e].b];
        // delta_g.rs:66-69: pairs never sent to ntthal when self-dimer checking is off
        if (!ntthal_pair_sent(a, b, cfg)) continue;
        g.edges[a].insert(b);
    }
    return g;
}

// --existing-primers: the candidates (one length) with a conflict against any panel primer, in either order of the
// pair -- run_ntthal's dG rule, screened as candidates x panel and panel x candidates (with --devices: on member 0;
// the block is at most 2,000 x the panel)
std::set<std::string> panel_conflicts(Engine &eng, const std::vector<std::string> &cands,
                                      const std::vector<std::string> &panel, const NtthalOptions &opts)
{
    std::set<std::string> out;
    if (cands.empty() || panel.empty()) return out;
    const int k = (int)cands[0].size(), nc = (int)cands.size(), np = (int)panel.size();
    std::string fc, fp;
    for (const auto &p : cands) fc += p;
    for (const auto &p : panel) fp += p;
    const msspe_chem chem = ntthal_chem(opts);
    for (int order = 0; order < 2; ++order) {   // 0: (candidate, panel), 1: (panel, candidate)
        const std::string &a = order ? fp : fc, &b = order ? fc : fp;
        const int na = order ? np : nc, nb = order ? nc : np;
        uint64_t count = 0;
        if (opts.use_end) {   // a 3'-end dimer with a panel primer in either role drops the candidate as well
            const msspe_conflict_rule rule = conflict_rule(opts);
            std::vector<msspe_kind_edge> kedges(4096);
            auto union_screen = [&]() {
                return msspe_conflict_graph_ab_edges(eng.ctx(), a.data(), na, k, b.data(), nb, k, &chem, &rule, kedges.data(),
                                                     kedges.size(), &count);
            };
            int rc = union_screen();
            if (rc == MSSPE_ERR_CAPACITY) {
                kedges.resize((size_t)count);
                rc = union_screen();
            }
            if (rc) eng.fail(rc);
            for (uint64_t e = 0; e < count; ++e) out.insert(cands[order ? kedges[(size_t)e].b : kedges[(size_t)e].a]);
            continue;
        }
        std::vector<msspe_edge> edges(4096);
        auto screen = [&]() {
            return msspe_cross_dimer_ab_edges(eng.ctx(), a.data(), na, k, b.data(), nb, k, &chem, opts.dg, edges.data(),
                                              edges.size(), &count);
        };
        int rc = screen();
        if (rc == MSSPE_ERR_CAPACITY) {
            edges.resize((size_t)count);
            rc = screen();
        }
        if (rc) eng.fail(rc);
        for (uint64_t e = 0; e < count; ++e) out.insert(cands[order ? edges[(size_t)e].b : edges[(size_t)e].a]);
    }
    return out;
}

std::pair<std::vector<std::string>, std::vector<std::string>> read_panel(const std::string &path, int kmer_size,
                                                                         const char *option)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw UsageError("error: cannot read '" + path + "' for '" + option + "'");
    std::pair<std::vector<std::string>, std::vector<std::string>> out;
    std::string line;
    size_t no = 0, col_dir = 0, col_primer = 2;
    auto split = [](const std::string &l) {
        std::vector<std::string> v;
        size_t at = 0;
        for (;;) {
            const size_t c = l.find(',', at);
            v.push_back(l.substr(at, c == std::string::npos ? std::string::npos : c - at));
            if (c == std::string::npos) return v;
            at = c + 1;
        }
    };
    while (std::getline(f, line)) {
        ++no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const std::string where = std::string("error: '") + option + "' " + path + " line " + std::to_string(no) + ": ";
        const auto fields = split(line);
        if (no == 1) {   // the header names the columns (direction,name,primers,gc,avg,std,tm)
            const auto d = std::find(fields.begin(), fields.end(), "direction");
            const auto p = std::find(fields.begin(), fields.end(), "primers");
            if (d == fields.end() || p == fields.end())
                throw UsageError(where + "the header has no 'direction' and 'primers' columns");
            col_dir = (size_t)(d - fields.begin());
            col_primer = (size_t)(p - fields.begin());
            continue;
        }
        if (line.empty()) continue;
        if (fields.size() <= std::max(col_dir, col_primer)) throw UsageError(where + "too few fields");
        const std::string &dir = fields[col_dir], &primer = fields[col_primer];
        if (dir != "F" && dir != "R") throw UsageError(where + "direction '" + dir + "' is neither F nor R");
        if (primer.size() != (size_t)kmer_size)
            throw UsageError(where + "primer '" + primer + "' has " + std::to_string(primer.size()) +
                             " bases, --kmer-size is " + std::to_string(kmer_size));
        if (primer.find_first_not_of("ACGT") != std::string::npos)
            throw UsageError(where + "primer '" + primer + "' holds characters other than A, C, G and T");
        (dir == "F" ? out.first : out.second).push_back(primer);
    }
    return out;
}

std::set<std::string> vertex_cover(const std::vector<std::string> &primers, const ConflictGraph &g)
{
    // main.rs:754-771: symmetric adjacency over conflict edges, self loops included
    std::map<std::string, std::set<std::string>> conflicts;
    for (const auto &p : primers) {
        auto it = g.edges.find(p);
        if (it != g.edges.end())
            for (const auto &b : it->second) {
                conflicts[p].insert(b);
                conflicts[b].insert(p);
            }
    }
    // main.rs:776-798: repeatedly delete the primer with most live conflicts; ties go to the
    // lexicographically greatest string.  Same rule on integer ids (the map iterates in
    // lexicographic order, so a node's id is its rank) with live degrees kept up to date.
    std::vector<const std::string *> name;
    std::map<std::string, int> id;
    for (const auto &kv : conflicts) {
        id.emplace(kv.first, (int)name.size());
        name.push_back(&kv.first);
    }
    const int n = (int)name.size();
    std::vector<std::vector<int>> adj((size_t)n);
    std::vector<int> live((size_t)n, 0);
    std::vector<char> gone((size_t)n, 0);
    for (const auto &kv : conflicts) {
        auto &list = adj[(size_t)id[kv.first]];
        for (const auto &nb : kv.second) list.push_back(id[nb]);
        live[(size_t)id[kv.first]] = (int)list.size();
    }
    std::set<std::string> deleted;
    for (;;) {
        int worst = -1;
        for (int v = 0; v < n; ++v)   // ascending rank: ">=" keeps the greatest string among equals
            if (!gone[(size_t)v] && live[(size_t)v] > 0 && (worst < 0 || live[(size_t)v] >= live[(size_t)worst])) worst = v;
        if (worst < 0) break;
        gone[(size_t)worst] = 1;
        deleted.insert(*name[(size_t)worst]);
        for (int nb : adj[(size_t)worst]) --live[(size_t)nb];   // conflicts are symmetric
    }
    return deleted;
}

std::set<std::string> conflict_cover_on_device(Engine &eng, const std::vector<std::string> &primers,
                                               const NtthalOptions &opts, const ProgramConfig &cfg)
{
    std::set<std::string> deleted;
    std::vector<std::string> nodes;   // run_ntthal's node list: duplicates collapse
    std::unordered_set<std::string> seen;
    for (const auto &p : primers)
        if (seen.insert(p).second) nodes.push_back(p);
    if (!cfg.check_cross_dimers || nodes.empty()) return deleted;   // delta_g.rs:71-73: no edges at all
    const int n = (int)nodes.size(), k = (int)nodes[0].size();
    std::string flat;
    for (const auto &p : nodes) flat += p;
    const msspe_chem chem = ntthal_chem(opts);
    std::vector<uint8_t> del((size_t)n);
    // --check-self-dimers false: the pairs ntthal_pair_sent() never sends are no edges
    const msspe_conflict_rule rule = conflict_rule(opts);
    const int rc = opts.use_end ? msspe_conflict_cover_rule(eng.ctx(), flat.data(), n, k, &chem, &rule,
                                                            cfg.check_self_dimers ? 0 : 1, del.data(), nullptr)
                                : msspe_conflict_cover(eng.ctx(), flat.data(), n, k, &chem, opts.dg,
                                                       cfg.check_self_dimers ? 0 : 1, del.data(), nullptr);
    if (rc) eng.fail(rc);
    if (opts.use_end) count_kinds(eng, flat, n, k, chem, opts);
    for (int i = 0; i < n; ++i)
        if (del[(size_t)i]) deleted.insert(nodes[(size_t)i]);
    return deleted;
}

std::map<std::string, int> assign_tubes(const std::vector<std::string> &primers, const ConflictGraph &g, int max_tubes)
{
    // the cover's graph (main.rs:754-771: symmetric, self loops kept) over the distinct primers; the set iterates in
    // lexicographic order, so a node's id is its rank
    const std::set<std::string> words(primers.begin(), primers.end());
    std::vector<const std::string *> name;
    std::map<std::string, int> id;
    for (const auto &w : words) {
        id.emplace(w, (int)name.size());
        name.push_back(&w);
    }
    const int n = (int)name.size();
    std::vector<std::set<int>> adj((size_t)n);
    std::vector<char> self((size_t)n, 0);
    for (const auto &kv : g.edges) {
        const auto a = id.find(kv.first);
        if (a == id.end()) continue;
        for (const auto &w : kv.second) {
            const auto b = id.find(w);
            if (b == id.end()) continue;
            if (a->second == b->second) self[(size_t)a->second] = 1;
            else {
                adj[(size_t)a->second].insert(b->second);
                adj[(size_t)b->second].insert(a->second);
            }
        }
    }
    std::vector<int> order;
    for (int v = 0; v < n; ++v)
        if (!self[(size_t)v]) order.push_back(v);
    std::sort(order.begin(), order.end(), [&](int a, int b) {   // descending (degree, rank)
        const size_t da = adj[(size_t)a].size(), db = adj[(size_t)b].size();
        return da != db ? da > db : a > b;
    });
    std::vector<int> tube((size_t)n, -1);
    for (int v : order) {
        uint64_t taken = 0;
        for (int u : adj[(size_t)v])
            if (tube[(size_t)u] >= 0) taken |= 1ull << tube[(size_t)u];
        for (int t = 0; t < max_tubes && t < 64; ++t)
            if (!((taken >> t) & 1)) {
                tube[(size_t)v] = t;
                break;
            }
    }
    std::map<std::string, int> out;
    for (int v = 0; v < n; ++v) out.emplace(*name[(size_t)v], tube[(size_t)v]);
    return out;
}

std::map<std::string, int> conflict_tubes_on_device(Engine &eng, const std::vector<std::string> &primers,
                                                    const NtthalOptions &opts, const ProgramConfig &cfg, int max_tubes)
{
    std::map<std::string, int> out;
    std::vector<std::string> nodes;   // run_ntthal's node list: duplicates collapse
    std::unordered_set<std::string> seen;
    for (const auto &p : primers)
        if (seen.insert(p).second) nodes.push_back(p);
    if (nodes.empty()) return out;
    if (!cfg.check_cross_dimers) {   // delta_g.rs:71-73: no edges at all, one tube holds everything
        for (const auto &p : nodes) out.emplace(p, 0);
        return out;
    }
    const int n = (int)nodes.size(), k = (int)nodes[0].size();
    std::string flat;
    for (const auto &p : nodes) flat += p;
    const msspe_chem chem = ntthal_chem(opts);
    std::vector<uint8_t> tube((size_t)n);
    // --check-self-dimers false: the pairs ntthal_pair_sent() never sends are no edges
    const msspe_conflict_rule rule = conflict_rule(opts);
    const int rc = opts.use_end ? msspe_conflict_tubes_rule(eng.ctx(), flat.data(), n, k, &chem, &rule,
                                                            cfg.check_self_dimers ? 0 : 1, max_tubes, tube.data(), nullptr,
                                                            nullptr)
                                : msspe_conflict_tubes(eng.ctx(), flat.data(), n, k, &chem, opts.dg,
                                                       cfg.check_self_dimers ? 0 : 1, max_tubes, tube.data(), nullptr, nullptr);
    if (rc) eng.fail(rc);
    if (opts.use_end) count_kinds(eng, flat, n, k, chem, opts);
    for (int i = 0; i < n; ++i)
        out.emplace(nodes[(size_t)i], tube[(size_t)i] == MSSPE_TUBE_NONE ? -1 : (int)tube[(size_t)i]);
    return out;
}

// the two additions of --thin-depth R to a thinning block; nothing at depth 1
static std::string thin_depth_tag(int depth) { return depth > 1 ? ", depth " + std::to_string(depth) : std::string(); }
static std::string thin_depth_line(int depth, size_t deep_all, size_t deep_kept, const std::string &t,
                                   const std::string &y, const std::string &x)
{
    if (depth <= 1) return std::string();
    return "  Depth:    at least " + std::to_string(depth) + " primers on " + std::to_string(deep_all) + "/" + t +
           " segments by all " + y + ", on " + std::to_string(deep_kept) + "/" + t + " by the kept " + x + "\n";
}

std::vector<char> thin_shadows(const std::vector<std::string> &fwd, const std::vector<std::string> &rev,
                               const std::vector<char> &forced)
{
    const size_t n = fwd.size() + rev.size();
    std::vector<char> shadow(n, 0);
    auto is_forced = [&](size_t p) { return p < forced.size() && forced[p]; };
    for (int dir = 0; dir < 2; ++dir) {   // a forward word that equals a reverse word is no duplicate
        const auto &words = dir ? rev : fwd;
        const size_t base = dir ? fwd.size() : 0;
        std::map<std::string, size_t> rep;   // word -> its representative so far
        for (size_t i = 0; i < words.size(); ++i) {
            const auto it = rep.find(words[i]);
            if (it == rep.end()) {
                rep.emplace(words[i], base + i);
            } else if (is_forced(base + i) && !is_forced(it->second)) {   // the first forced one takes over
                shadow[it->second] = 1;
                it->second = base + i;
            } else {
                shadow[base + i] = 1;
            }
        }
    }
    return shadow;
}

ThinDepthResult thin_panel_depth(const std::vector<std::vector<uint64_t>> &rows, size_t n_seg, int depth, int min_gain,
                                 const std::vector<char> &forced, const std::vector<char> &shadow)
{
    const size_t n = rows.size();
    auto bit = [&](size_t p, size_t s) { return (s >> 6) < rows[p].size() && ((rows[p][s >> 6] >> (s & 63)) & 1ull); };
    auto is_forced = [&](size_t p) { return p < forced.size() && forced[p]; };
    auto is_shadow = [&](size_t p) { return p < shadow.size() && shadow[p]; };
    ThinDepthResult out;
    out.keep.assign(n, 0);
    std::vector<int> all(n_seg, 0), need(n_seg, 0), cnt(n_seg, 0);
    for (size_t p = 0; p < n; ++p) {
        out.keep[p] = is_forced(p) ? 1 : 0;
        if (is_shadow(p)) continue;
        for (size_t s = 0; s < n_seg; ++s)
            if (bit(p, s)) {
                ++all[s];
                if (is_forced(p)) ++cnt[s];
            }
    }
    for (size_t s = 0; s < n_seg; ++s) {
        need[s] = std::min(depth, all[s]);
        cnt[s] = std::min(need[s], cnt[s]);
    }
    for (;;) {   // every round from scratch: the device keeps its gains up to date instead
        long best = -1;
        size_t best_gain = 0;
        for (size_t p = 0; p < n; ++p) {
            if (out.keep[p] || is_shadow(p)) continue;
            size_t gain = 0;
            for (size_t s = 0; s < n_seg; ++s) gain += bit(p, s) && cnt[s] < need[s] ? 1 : 0;
            if (best < 0 || gain > best_gain) {   // ">": the lowest index among equals
                best = (long)p;
                best_gain = gain;
            }
        }
        ++out.rounds;
        if (best < 0 || best_gain < (size_t)min_gain) break;
        out.order.push_back((int)best);
        out.gains.push_back((int)best_gain);
        out.keep[(size_t)best] = 1;
        for (size_t s = 0; s < n_seg; ++s)
            if (bit((size_t)best, s) && cnt[s] < need[s]) ++cnt[s];
    }
    out.depth_all.assign(n_seg, 0);
    out.depth_kept.assign(n_seg, 0);
    for (size_t s = 0; s < n_seg; ++s) {
        int kept = 0;
        for (size_t p = 0; p < n; ++p) kept += out.keep[p] && !is_shadow(p) && bit(p, s) ? 1 : 0;
        out.depth_all[s] = (uint8_t)std::min(all[s], 255);
        out.depth_kept[s] = (uint8_t)std::min(kept, 255);
        out.counts[0] += all[s] >= 1;
        out.counts[1] += kept >= 1;
        out.counts[2] += all[s] >= depth;
        out.counts[3] += kept >= depth;
    }
    return out;
}

// a round's gain from one word of a row: the new bits' number, or with weights (one per segment) their weights' sum
static size_t word_gain(uint64_t bits, size_t w, const std::vector<uint32_t> *weights)
{
    if (!weights) return (size_t)__builtin_popcountll(bits);
    size_t sum = 0;
    for (; bits; bits &= bits - 1) {
        const size_t s = w * 64 + (size_t)__builtin_ctzll(bits);
        if (s < weights->size()) sum += (*weights)[s];
    }
    return sum;
}

// weight_all / weight_kept of a weighted run from the words covered by all rows and by the kept ones
static void weigh_cover(const std::vector<uint64_t> &all, const std::vector<uint64_t> &covered,
                        const std::vector<uint32_t> &weights, WeightedSums &sums)
{
    for (size_t w = 0; w < all.size(); ++w) {
        sums.weight_all += word_gain(all[w], w, &weights);
        sums.weight_kept += word_gain(covered[w], w, &weights);
    }
}

// thin_panel, and with weights thin_panel_weighted: the gains go to sums->gains then, out.gains stays empty
static ThinResult thin_panel_rule(const std::vector<std::vector<uint64_t>> &rows, long long min_gain,
                                  const std::vector<char> &forced, const std::vector<uint32_t> *weights,
                                  WeightedSums *sums)
{
    const size_t n = rows.size();
    size_t words = 0;
    for (const auto &r : rows) words = std::max(words, r.size());
    auto word = [&](size_t p, size_t w) { return w < rows[p].size() ? rows[p][w] : 0ull; };
    ThinResult out;
    out.keep.assign(n, 0);
    std::vector<uint64_t> covered(words, 0), all(words, 0);
    for (size_t p = 0; p < n; ++p)
        for (size_t w = 0; w < words; ++w) {
            all[w] |= word(p, w);
            if (p < forced.size() && forced[p]) covered[w] |= word(p, w);
        }
    for (size_t p = 0; p < n; ++p) out.keep[p] = p < forced.size() && forced[p] ? 1 : 0;
    for (;;) {   // every round from scratch: the device keeps its gains up to date instead
        long best = -1;
        size_t best_gain = 0;
        for (size_t p = 0; p < n; ++p) {
            if (out.keep[p]) continue;
            size_t gain = 0;
            for (size_t w = 0; w < words; ++w) gain += word_gain(word(p, w) & ~covered[w], w, weights);
            if (best < 0 || gain > best_gain) {   // ">": the lowest index among equals
                best = (long)p;
                best_gain = gain;
            }
        }
        if (best < 0 || best_gain < (size_t)min_gain) break;
        out.order.push_back((int)best);
        if (weights) sums->gains.push_back((uint32_t)best_gain);
        else out.gains.push_back((int)best_gain);
        out.keep[(size_t)best] = 1;
        for (size_t w = 0; w < words; ++w) covered[w] |= word((size_t)best, w);
    }
    for (size_t w = 0; w < words; ++w) {
        out.covered_all += (size_t)__builtin_popcountll(all[w]);
        out.covered_kept += (size_t)__builtin_popcountll(covered[w]);
    }
    if (weights) weigh_cover(all, covered, *weights, *sums);
    return out;
}

ThinResult thin_panel(const std::vector<std::vector<uint64_t>> &rows, int min_gain, const std::vector<char> &forced)
{
    return thin_panel_rule(rows, min_gain, forced, nullptr, nullptr);
}

ThinResult thin_panel_weighted(const std::vector<std::vector<uint64_t>> &rows, const std::vector<uint32_t> &weights,
                               long long min_gain, const std::vector<char> &forced, WeightedSums &sums)
{
    sums = WeightedSums{};
    return thin_panel_rule(rows, min_gain, forced, &weights, &sums);
}

// the cover's graph over the primers' indices: symmetric, a self loop kept apart
static void select_graph(const std::vector<std::string> &primers, const ConflictGraph &g,
                         std::vector<std::set<size_t>> &adj, std::vector<char> &self)
{
    const size_t n = primers.size();
    std::map<std::string, size_t> id;
    for (size_t p = 0; p < n; ++p) id.emplace(primers[p], p);
    adj.assign(n, {});
    self.assign(n, 0);
    for (const auto &kv : g.edges) {
        const auto a = id.find(kv.first);
        if (a == id.end()) continue;
        for (const auto &w : kv.second) {
            const auto b = id.find(w);
            if (b == id.end()) continue;
            if (a->second == b->second) self[a->second] = 1;
            else {
                adj[a->second].insert(b->second);
                adj[b->second].insert(a->second);
            }
        }
    }
}

SelectDepthResult select_panel_depth(const std::vector<std::vector<uint64_t>> &rows,
                                     const std::vector<std::string> &primers, const ConflictGraph &g, size_t n_seg,
                                     int depth, int max_tubes, int min_gain, const std::vector<char> &forced)
{
    const size_t n = rows.size();
    auto bit = [&](size_t p, size_t s) { return (s >> 6) < rows[p].size() && ((rows[p][s >> 6] >> (s & 63)) & 1ull); };
    auto is_forced = [&](size_t p) { return p < forced.size() && forced[p]; };
    std::vector<std::set<size_t>> adj;
    std::vector<char> self;
    select_graph(primers, g, adj, self);
    const uint64_t all_tubes = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    SelectDepthResult out;
    out.keep.assign(n, 0);
    out.tube.assign(n, -1);
    out.barred.assign(n, 0);
    std::vector<int> all(n_seg, 0), cnt(n_seg, 0);   // the true counts
    std::vector<uint64_t> mask(n, 0);
    int deepest = 0;
    for (size_t p = 0; p < n; ++p) {
        out.keep[p] = is_forced(p) ? 1 : 0;
        for (size_t s = 0; s < n_seg; ++s)
            if (bit(p, s)) {
                ++all[s];
                if (is_forced(p)) ++cnt[s];
            }
        if (is_forced(p))   // the panel is in every tube
            for (size_t u : adj[p]) mask[u] = all_tubes;
    }
    for (size_t s = 0; s < n_seg; ++s) deepest = std::max(deepest, all[s]);
    out.layers = std::min(depth, std::max(1, deepest));
    for (int r = 1; r <= out.layers; ++r)
        for (;;) {   // every round from scratch: the device keeps its gains up to date instead
            long best = -1;
            size_t best_gain = 0;
            for (size_t p = 0; p < n; ++p) {
                if (out.keep[p] || self[p] || (mask[p] & all_tubes) == all_tubes) continue;
                size_t gain = 0;
                for (size_t s = 0; s < n_seg; ++s) gain += bit(p, s) && cnt[s] < std::min(r, all[s]) ? 1 : 0;
                if (best < 0 || gain > best_gain) {   // ">": the lowest index among equals
                    best = (long)p;
                    best_gain = gain;
                }
            }
            ++out.rounds;
            if (best < 0 || best_gain < (size_t)min_gain) break;   // the layer ends
            const size_t p = (size_t)best;
            const int t = __builtin_ctzll(~mask[p] & all_tubes);
            out.order.push_back((int)best);
            out.gains.push_back((int)best_gain);
            out.layer.push_back(r);
            out.keep[p] = 1;
            out.tube[p] = t;
            out.tubes_used = std::max(out.tubes_used, t + 1);
            for (size_t s = 0; s < n_seg; ++s)
                if (bit(p, s)) ++cnt[s];   // open or not
            for (size_t u : adj[p]) mask[u] |= 1ull << t;
        }
    for (size_t p = 0; p < n; ++p)
        out.barred[p] = !out.keep[p] && (self[p] || (mask[p] & all_tubes) == all_tubes) ? 1 : 0;
    out.depth_all.assign(n_seg, 0);
    out.depth_kept.assign(n_seg, 0);
    for (size_t s = 0; s < n_seg; ++s) {
        out.depth_all[s] = (uint8_t)std::min(all[s], 255);
        out.depth_kept[s] = (uint8_t)std::min(cnt[s], 255);
        out.counts[0] += all[s] >= 1;
        out.counts[1] += cnt[s] >= 1;
        out.counts[2] += all[s] >= depth;
        out.counts[3] += cnt[s] >= depth;
    }
    return out;
}

// select_panel, and with weights select_panel_weighted: the gains go to sums->gains then, out.gains stays empty
static SelectResult select_panel_rule(const std::vector<std::vector<uint64_t>> &rows,
                                      const std::vector<std::string> &primers, const ConflictGraph &g, int max_tubes,
                                      long long min_gain, const std::vector<char> &forced,
                                      const std::vector<uint32_t> *weights, WeightedSums *sums)
{
    const size_t n = rows.size();
    size_t words = 0;
    for (const auto &r : rows) words = std::max(words, r.size());
    auto word = [&](size_t p, size_t w) { return w < rows[p].size() ? rows[p][w] : 0ull; };
    auto is_forced = [&](size_t p) { return p < forced.size() && forced[p]; };
    std::vector<std::set<size_t>> adj;
    std::vector<char> self;
    select_graph(primers, g, adj, self);
    const uint64_t all_tubes = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    SelectResult out;
    out.keep.assign(n, 0);
    out.tube.assign(n, -1);
    out.barred.assign(n, 0);
    std::vector<uint64_t> covered(words, 0), all(words, 0), mask(n, 0);
    for (size_t p = 0; p < n; ++p) {
        out.keep[p] = is_forced(p) ? 1 : 0;
        for (size_t w = 0; w < words; ++w) {
            all[w] |= word(p, w);
            if (is_forced(p)) covered[w] |= word(p, w);
        }
        if (is_forced(p))   // the panel is in every tube
            for (size_t u : adj[p]) mask[u] = all_tubes;
    }
    for (;;) {   // every round from scratch: the device keeps its gains up to date instead
        long best = -1;
        size_t best_gain = 0;
        for (size_t p = 0; p < n; ++p) {
            if (out.keep[p] || self[p] || (mask[p] & all_tubes) == all_tubes) continue;
            size_t gain = 0;
            for (size_t w = 0; w < words; ++w) gain += word_gain(word(p, w) & ~covered[w], w, weights);
            if (best < 0 || gain > best_gain) {   // ">": the lowest index among equals
                best = (long)p;
                best_gain = gain;
            }
        }
        ++out.rounds;
        if (best < 0 || best_gain < (size_t)min_gain) break;
        const size_t p = (size_t)best;
        const int t = __builtin_ctzll(~mask[p] & all_tubes);
        out.order.push_back((int)best);
        if (weights) sums->gains.push_back((uint32_t)best_gain);
        else out.gains.push_back((int)best_gain);
        out.keep[p] = 1;
        out.tube[p] = t;
        out.tubes_used = std::max(out.tubes_used, t + 1);
        for (size_t w = 0; w < words; ++w) covered[w] |= word(p, w);
        for (size_t u : adj[p]) mask[u] |= 1ull << t;
    }
    for (size_t p = 0; p < n; ++p)
        out.barred[p] = !out.keep[p] && (self[p] || (mask[p] & all_tubes) == all_tubes) ? 1 : 0;
    for (size_t w = 0; w < words; ++w) {
        out.covered_all += (size_t)__builtin_popcountll(all[w]);
        out.covered_kept += (size_t)__builtin_popcountll(covered[w]);
    }
    out.covered = covered;
    if (weights) weigh_cover(all, covered, *weights, *sums);
    return out;
}

SelectResult select_panel(const std::vector<std::vector<uint64_t>> &rows, const std::vector<std::string> &primers,
                          const ConflictGraph &g, int max_tubes, int min_gain, const std::vector<char> &forced)
{
    return select_panel_rule(rows, primers, g, max_tubes, min_gain, forced, nullptr, nullptr);
}

SelectResult select_panel_weighted(const std::vector<std::vector<uint64_t>> &rows,
                                   const std::vector<std::string> &primers, const ConflictGraph &g,
                                   const std::vector<uint32_t> &weights, int max_tubes, long long min_gain,
                                   const std::vector<char> &forced, WeightedSums &sums)
{
    sums = WeightedSums{};
    return select_panel_rule(rows, primers, g, max_tubes, min_gain, forced, &weights, &sums);
}

// a beats b under the cost rule: the greater gain / cost by the cross products (gains and costs are below 2^32, so
// the products are exact in 64 bits), then the greater gain; the caller walks by ascending index and asks "beats"
// strictly, which leaves the lowest index among equals
static bool cost_beats(uint64_t gain_a, uint32_t cost_a, uint64_t gain_b, uint32_t cost_b)
{
    const uint64_t ab = gain_a * (uint64_t)cost_b, ba = gain_b * (uint64_t)cost_a;
    return ab != ba ? ab > ba : gain_a > gain_b;
}

// what both cost twins end with: the two cost sums, and the two weights (without weights: the two covered counts)
static void cost_sums(const std::vector<char> &keep, const std::vector<uint32_t> &costs,
                      const std::vector<uint64_t> &all, const std::vector<uint64_t> &covered,
                      const std::vector<uint32_t> *weights, size_t covered_all, size_t covered_kept, CostSums &sums)
{
    for (size_t p = 0; p < keep.size(); ++p) {
        sums.cost_all += costs[p];
        if (keep[p]) sums.cost_kept += costs[p];
    }
    if (!weights) {
        sums.weight_all = covered_all;
        sums.weight_kept = covered_kept;
        return;
    }
    for (size_t w = 0; w < all.size(); ++w) {
        sums.weight_all += word_gain(all[w], w, weights);
        sums.weight_kept += word_gain(covered[w], w, weights);
    }
}

ThinResult thin_panel_cost(const std::vector<std::vector<uint64_t>> &rows, const std::vector<uint32_t> *weights,
                           const std::vector<uint32_t> &costs, long long min_gain, const std::vector<char> &forced,
                           CostSums &sums)
{
    sums = CostSums{};
    const size_t n = rows.size();
    size_t words = 0;
    for (const auto &r : rows) words = std::max(words, r.size());
    auto word = [&](size_t p, size_t w) { return w < rows[p].size() ? rows[p][w] : 0ull; };
    ThinResult out;
    out.keep.assign(n, 0);
    std::vector<uint64_t> covered(words, 0), all(words, 0);
    for (size_t p = 0; p < n; ++p) {
        out.keep[p] = p < forced.size() && forced[p] ? 1 : 0;
        for (size_t w = 0; w < words; ++w) {
            all[w] |= word(p, w);
            if (out.keep[p]) covered[w] |= word(p, w);
        }
    }
    for (;;) {   // every round from scratch: the device keeps its gains up to date instead
        long best = -1;
        uint64_t best_gain = 0;
        for (size_t p = 0; p < n; ++p) {
            if (out.keep[p]) continue;
            uint64_t gain = 0;
            for (size_t w = 0; w < words; ++w) gain += word_gain(word(p, w) & ~covered[w], w, weights);
            if ((long long)gain < min_gain) continue;   // no candidate, whatever its ratio
            if (best < 0 || cost_beats(gain, costs[p], best_gain, costs[(size_t)best])) {
                best = (long)p;
                best_gain = gain;
            }
        }
        if (best < 0) break;
        out.order.push_back((int)best);
        sums.gains.push_back((uint32_t)best_gain);
        out.keep[(size_t)best] = 1;
        for (size_t w = 0; w < words; ++w) covered[w] |= word((size_t)best, w);
    }
    for (size_t w = 0; w < words; ++w) {
        out.covered_all += (size_t)__builtin_popcountll(all[w]);
        out.covered_kept += (size_t)__builtin_popcountll(covered[w]);
    }
    cost_sums(out.keep, costs, all, covered, weights, out.covered_all, out.covered_kept, sums);
    return out;
}

SelectResult select_panel_cost(const std::vector<std::vector<uint64_t>> &rows, const std::vector<std::string> &primers,
                               const ConflictGraph &g, const std::vector<uint32_t> *weights,
                               const std::vector<uint32_t> &costs, int max_tubes, long long min_gain,
                               const std::vector<char> &forced, CostSums &sums)
{
    sums = CostSums{};
    const size_t n = rows.size();
    size_t words = 0;
    for (const auto &r : rows) words = std::max(words, r.size());
    auto word = [&](size_t p, size_t w) { return w < rows[p].size() ? rows[p][w] : 0ull; };
    auto is_forced = [&](size_t p) { return p < forced.size() && forced[p]; };
    std::vector<std::set<size_t>> adj;
    std::vector<char> self;
    select_graph(primers, g, adj, self);
    const uint64_t all_tubes = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    SelectResult out;
    out.keep.assign(n, 0);
    out.tube.assign(n, -1);
    out.barred.assign(n, 0);
    std::vector<uint64_t> covered(words, 0), all(words, 0), mask(n, 0);
    for (size_t p = 0; p < n; ++p) {
        out.keep[p] = is_forced(p) ? 1 : 0;
        for (size_t w = 0; w < words; ++w) {
            all[w] |= word(p, w);
            if (is_forced(p)) covered[w] |= word(p, w);
        }
        if (is_forced(p))   // the panel is in every tube
            for (size_t u : adj[p]) mask[u] = all_tubes;
    }
    for (;;) {   // every round from scratch: the device keeps its gains up to date instead
        long best = -1;
        uint64_t best_gain = 0;
        for (size_t p = 0; p < n; ++p) {
            if (out.keep[p] || self[p] || (mask[p] & all_tubes) == all_tubes) continue;
            uint64_t gain = 0;
            for (size_t w = 0; w < words; ++w) gain += word_gain(word(p, w) & ~covered[w], w, weights);
            if ((long long)gain < min_gain) continue;   // no candidate, whatever its ratio
            if (best < 0 || cost_beats(gain, costs[p], best_gain, costs[(size_t)best])) {
                best = (long)p;
                best_gain = gain;
            }
        }
        ++out.rounds;
        if (best < 0) break;
        const size_t p = (size_t)best;
        const int t = __builtin_ctzll(~mask[p] & all_tubes);
        out.order.push_back((int)best);
        sums.gains.push_back((uint32_t)best_gain);
        out.keep[p] = 1;
        out.tube[p] = t;
        out.tubes_used = std::max(out.tubes_used, t + 1);
        for (size_t w = 0; w < words; ++w) covered[w] |= word(p, w);
        for (size_t u : adj[p]) mask[u] |= 1ull << t;
    }
    for (size_t p = 0; p < n; ++p)
        out.barred[p] = !out.keep[p] && (self[p] || (mask[p] & all_tubes) == all_tubes) ? 1 : 0;
    for (size_t w = 0; w < words; ++w) {
        out.covered_all += (size_t)__builtin_popcountll(all[w]);
        out.covered_kept += (size_t)__builtin_popcountll(covered[w]);
    }
    out.covered = covered;
    cost_sums(out.keep, costs, all, covered, weights, out.covered_all, out.covered_kept, sums);
    return out;
}

std::string cost_line(uint64_t cost_kept, uint64_t cost_all, size_t n_kept, size_t n_all)
{
    return "  Cost:     " + std::to_string(cost_kept) + "/" + std::to_string(cost_all) + " by the kept " +
           std::to_string(n_kept) + " of " + std::to_string(n_all) + "\n";
}

std::map<std::string, uint32_t> read_primer_costs(const std::string &path, int kmer_size)
{
    const char *option = "--primer-costs";
    std::ifstream f(path, std::ios::binary);
    if (!f) throw UsageError(std::string("error: cannot read '") + path + "' for '" + option + "'");
    const uint64_t limit = 0xFFFFFFFFull;
    std::map<std::string, uint32_t> out;
    std::string line;
    size_t no = 0;
    while (std::getline(f, line)) {
        ++no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string where = std::string("error: '") + option + "' " + path + " line " + std::to_string(no) + ": ";
        const size_t c = line.find(',');
        if (c == std::string::npos || c == 0 || line.find(',', c + 1) != std::string::npos)
            throw UsageError(where + "expected 'sequence,cost'");
        const std::string seq = line.substr(0, c), text = line.substr(c + 1);
        if (seq.size() != (size_t)kmer_size || seq.find_first_not_of("ACGT") != std::string::npos)
            throw UsageError(where + "sequence '" + seq + "' is not " + std::to_string(kmer_size) +
                             " bases of A, C, G, T ('--kmer-size')");
        char *end = nullptr;
        errno = 0;
        const unsigned long long x = std::strtoull(text.c_str(), &end, 10);
        if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos || *end || errno || x < 1 ||
            x > limit)
            throw UsageError(where + "cost '" + text + "' is not an integer in 1 .. " + std::to_string(limit));
        out[seq] = (uint32_t)x;   // a sequence listed again: the later line holds
    }
    return out;
}

uint32_t primer_cost(uint32_t base, uint32_t per_site, uint64_t sites)
{
    const uint64_t limit = 0xFFFFFFFFull;
    if (per_site && sites > limit / per_site) return (uint32_t)limit;   // the product alone is past the limit
    return (uint32_t)std::min<uint64_t>(limit, (uint64_t)base + (uint64_t)per_site * sites);
}

std::string weight_line(uint64_t weight_all, uint64_t weight_kept, uint64_t weight_total, size_t n_all, size_t n_kept)
{
    const std::string t = std::to_string(weight_total);
    return "  Weight:   covered " + std::to_string(weight_all) + "/" + t + " by all " + std::to_string(n_all) + ", " +
           std::to_string(weight_kept) + "/" + t + " by the kept " + std::to_string(n_kept) + "\n";
}

// a thinning or selection block with `line` put in behind its "  Segments:" line
static std::string with_weight_line(std::string block, const std::string &line)
{
    const size_t at = block.find("\n  Segments:");
    const size_t end = at == std::string::npos ? std::string::npos : block.find('\n', at + 1);
    if (end != std::string::npos) block.insert(end + 1, line);
    return block;
}

std::vector<uint32_t> read_genome_weights(const std::string &path, const std::vector<SequenceRecord> &records,
                                          int default_weight, size_t partitions)
{
    const char *option = "--genome-weights";
    std::ifstream f(path, std::ios::binary);
    if (!f) throw UsageError(std::string("error: cannot read '") + path + "' for '" + option + "'");
    const uint64_t limit = 0xFFFFFFFFull;
    std::map<std::string, std::vector<size_t>> by_name;   // a name that several records carry applies to all of them
    for (size_t r = 0; r < records.size(); ++r) by_name[records[r].name].push_back(r);
    std::vector<uint32_t> out(records.size(), (uint32_t)default_weight);
    std::vector<char> listed(records.size(), 0);
    uint64_t total = 0;   // over the listed records' segments, line by line
    std::string line;
    size_t no = 0;
    while (std::getline(f, line)) {
        ++no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string where = std::string("error: '") + option + "' " + path + " line " + std::to_string(no) + ": ";
        const size_t c = line.rfind(',');   // the weight is the last field: a record's name may hold commas
        if (c == std::string::npos || c == 0) throw UsageError(where + "expected 'name,weight'");
        const std::string name = line.substr(0, c), text = line.substr(c + 1);
        char *end = nullptr;
        errno = 0;
        const unsigned long long x = std::strtoull(text.c_str(), &end, 10);
        if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos || *end || errno || x > limit)
            throw UsageError(where + "weight '" + text + "' is not an integer in 0 .. " + std::to_string(limit));
        const auto it = by_name.find(name);
        if (it == by_name.end()) throw UsageError(where + "no record is named '" + name + "'");
        for (const size_t r : it->second) {
            if (listed[r]) total -= (uint64_t)out[r] * partitions;   // a name listed again: the later line holds
            out[r] = (uint32_t)x;
            listed[r] = 1;
            total += x * partitions;
        }
        if (total > limit)
            throw UsageError(where + "the weights add up to " + std::to_string(total) + " over " +
                             std::to_string(partitions) + " segments per record, at most " + std::to_string(limit));
    }
    for (size_t r = 0; r < records.size(); ++r)
        if (!listed[r]) total += (uint64_t)default_weight * partitions;
    if (total > limit)
        throw UsageError(std::string("error: '") + option + "' " + path + ": with '--default-genome-weight " +
                         std::to_string(default_weight) + "' on the records it does not list the weights add up to " +
                         std::to_string(total) + ", at most " + std::to_string(limit));
    return out;
}

std::string thin_report(int max_mismatches, int exact_3p, int min_gain, size_t kept_f, size_t n_f, size_t kept_r,
                        size_t n_r, size_t forced, size_t covered_all, size_t covered_kept, size_t segments,
                        int depth, size_t deep_all, size_t deep_kept)
{
    const std::string x = std::to_string(kept_f + kept_r), y = std::to_string(n_f + n_r), t = std::to_string(segments);
    return "\nPanel thinning (up to " + std::to_string(max_mismatches) + " mismatches, last " + std::to_string(exact_3p) +
           " bases exact, gain >= " + std::to_string(min_gain) + thin_depth_tag(depth) + "):\n  Primers:  kept " + x +
           " of " + y + " (forward " +
           std::to_string(kept_f) + " of " + std::to_string(n_f) + ", reverse " + std::to_string(kept_r) + " of " +
           std::to_string(n_r) + "), " + std::to_string(forced) + " forced\n  Segments: covered " +
           std::to_string(covered_all) + "/" + t + " by all " + y + ", " + std::to_string(covered_kept) + "/" + t +
           " by the kept " + x + "\n" + thin_depth_line(depth, deep_all, deep_kept, t, y, x);
}

std::string tubes_report(const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                         const std::map<std::string, int> &tubes, int max_tubes)
{
    std::vector<size_t> count;
    size_t unplaced = 0;
    for (const auto *list : {&fwd, &rev})
        for (const auto &p : *list) {
            const auto it = tubes.find(p.word);
            if (it == tubes.end() || it->second < 0) {
                ++unplaced;
                continue;
            }
            if (count.size() <= (size_t)it->second) count.resize((size_t)it->second + 1, 0);
            ++count[(size_t)it->second];
        }
    std::string out = "Tube assignment (up to " + std::to_string(max_tubes) + " tubes):\n  Tubes used: " +
                      std::to_string(count.size()) + "\n";
    for (size_t t = 0; t < count.size(); ++t)
        out += "  Tube " + std::to_string(t + 1) + ": " + std::to_string(count[t]) + " primers\n";
    out += "  Unplaced: " + std::to_string(unplaced) + " primers\n";
    return out;
}

// ---------------------------------------------------------------------------------------------
// report + CSV (main.rs:518-594, 834-858): host-side text
// ---------------------------------------------------------------------------------------------
namespace {

std::string fmt(const char *f, double v)
{
    char b[64];
    std::snprintf(b, sizeof b, f, v);
    return b;
}

std::vector<uint64_t> pack_words(Engine &eng, const std::vector<KmerStat> &list, int k)
{
    std::vector<uint64_t> out(list.size());
    if (list.empty()) return out;
    std::string flat;
    for (const auto &p : list) flat += p.word;
    const int rc = msspe_pack_oligos(flat.data(), (int)list.size(), k, out.data());
    if (rc) eng.fail(rc);
    return out;
}

}  // namespace

namespace {
// The three lines of main.rs:574-593 under a heading: segments covered, sequences at >= 80 %, uncovered partitions.
// covered_at(record * P + partition): the rule the caller counts by (segments past a short record's end are not
// counted, as the reference's partitions of that record).
template <typename Covered>
std::string coverage_lines(const std::vector<SequenceRecord> &records, size_t P, int segment_size, int overlap_size,
                           Covered covered_at)
{
    size_t total = 0, covered = 0;
    std::map<std::string, std::pair<size_t, size_t>> seq_stats;        // name -> (covered, total)
    std::map<uint16_t, std::pair<size_t, size_t>> partition_stats;
    for (size_t ri = 0; ri < records.size(); ++ri) {
        const auto &r = records[ri];
        const size_t len = r.sequence.size();
        auto &se = seq_stats[r.name];
        for (size_t j = 0; (size_t)segment_size <= len && j * (size_t)overlap_size + (size_t)segment_size <= len; ++j) {
            const bool h = covered_at(ri * P + j);
            auto &pe = partition_stats[(uint16_t)j];
            se.second += 1;
            pe.second += 1;
            total += 1;
            if (h) {
                se.first += 1;
                pe.first += 1;
                covered += 1;
            }
        }
    }
    float min_cov = INFINITY, max_cov = -INFINITY;
    size_t well = 0;
    for (const auto &kv : seq_stats) {
        const float c = (float)kv.second.first / (float)kv.second.second * 100.0f;
        min_cov = std::fmin(min_cov, c);
        max_cov = std::fmax(max_cov, c);
        if (c >= 80.0f) ++well;
    }
    std::string out = "  Segments:  " + std::to_string(covered) + "/" + std::to_string(total) + " covered (" +
           fmt("%.1f", (double)(100.0f * (float)covered / (float)total)) + "%)\n";
    out += "  Sequences: " + std::to_string(well) + "/" + std::to_string(seq_stats.size()) +
           " at \xe2\x89\xa5" "80% coverage (min " + fmt("%.1f", (double)min_cov) + "%, max " +
           fmt("%.1f", (double)max_cov) + "%)\n";
    std::string unc;
    for (const auto &kv : partition_stats)
        if (kv.second.first == 0) unc += (unc.empty() ? "" : ", ") + std::to_string(kv.first);
    if (unc.empty()) out += "  All partitions have primer coverage\n";
    else out += "  Uncovered partitions: [" + unc + "]\n";
    return out;
}
}  // namespace

std::string coverage_report(Engine &eng, const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                            const std::vector<SequenceRecord> &records, int segment_size,
                            int overlap_size, int window_size, int kmer_size)
{
    const DeviceAlignment aln(eng, records);
    return coverage_report(eng, aln, fwd, rev, records, segment_size, overlap_size, window_size, kmer_size);
}

std::string coverage_report(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                            const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                            int segment_size, int overlap_size, int window_size, int kmer_size)
{
    // per-segment search on the device: hit[record * P + partition]
    const size_t L = aln.length();
    const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
    std::vector<uint8_t> hit(records.size() * P + 1);
    if (P) {
        const auto wf = pack_words(eng, fwd, kmer_size), wr = pack_words(eng, rev, kmer_size);
        msspe_kmer_opt opt{segment_size, overlap_size, window_size, kmer_size, 0, 0};
        const int rc = msspe_segment_coverage_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, wf.data(),
                                                  (int)wf.size(), wr.data(), (int)wr.size(), hit.data());
        if (rc) eng.fail(rc);
    }
    std::string out = "\nCoverage report:\n";
    out += coverage_lines(records, P, segment_size, overlap_size, [&](size_t i) { return hit[i] != 0; });
    return out;
}

std::string coverage_report_mm(Engine &eng, const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev,
                               const std::vector<SequenceRecord> &records, int segment_size, int overlap_size,
                               int window_size, int kmer_size, int max_mismatches, int exact_3p)
{
    const DeviceAlignment aln(eng, records);
    return coverage_report_mm(eng, aln, fwd, rev, records, segment_size, overlap_size, window_size, kmer_size,
                              max_mismatches, exact_3p);
}

std::string coverage_report_mm(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                               const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                               int segment_size, int overlap_size, int window_size, int kmer_size, int max_mismatches,
                               int exact_3p)
{
    // per-segment best mismatch count on the device: best[record * P + partition], 255 = no match
    const size_t L = aln.length();
    const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
    std::vector<uint8_t> best(records.size() * P + 1, 255);
    if (P) {
        const auto wf = pack_words(eng, fwd, kmer_size), wr = pack_words(eng, rev, kmer_size);
        const msspe_kmer_opt opt{segment_size, overlap_size, window_size, kmer_size, 0, 0};
        const msspe_mismatch_opt mm{max_mismatches, exact_3p};
        const int rc = msspe_segment_coverage_mm_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm,
                                                            wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                            best.data(), nullptr);
        if (rc) eng.fail(rc);
    }
    const auto n = (uint8_t)max_mismatches;
    std::string out = "\nCoverage report (up to " + std::to_string(max_mismatches) + " mismatches, last " +
                      std::to_string(exact_3p) + " bases exact):\n";
    out += coverage_lines(records, P, segment_size, overlap_size, [&](size_t i) { return best[i] <= n; });
    std::vector<size_t> by((size_t)max_mismatches + 2, 0);   // [0..N] mismatches, [N + 1] none
    for (size_t ri = 0; ri < records.size(); ++ri) {
        const size_t len = records[ri].sequence.size();
        for (size_t j = 0; (size_t)segment_size <= len && j * (size_t)overlap_size + (size_t)segment_size <= len; ++j)
            by[std::min<size_t>(best[ri * P + j], (size_t)max_mismatches + 1)] += 1;
    }
    out += "  Segments by best match:";
    for (int m = 0; m <= max_mismatches; ++m) out += " " + std::to_string(m) + " mm " + std::to_string(by[(size_t)m]) + ",";
    out += " none " + std::to_string(by.back()) + "\n";
    return out;
}

std::string coverage_thal_block(const std::vector<SequenceRecord> &records, size_t P, int segment_size,
                                int overlap_size, const uint8_t *held, const uint32_t *primer_held, size_t n_primers,
                                int max_mismatches, int exact_3p, int mode, float tm_threshold)
{
    size_t total = 0, n_held = 0, matched = 0;
    std::map<std::string, std::pair<size_t, size_t>> seq_stats;   // name -> (held, total)
    for (size_t ri = 0; ri < records.size(); ++ri) {
        const size_t len = records[ri].sequence.size();
        auto &se = seq_stats[records[ri].name];
        for (size_t j = 0; (size_t)segment_size <= len && j * (size_t)overlap_size + (size_t)segment_size <= len; ++j) {
            const uint8_t h = held[ri * P + j];
            se.second += 1;
            total += 1;
            if (h) matched += 1;
            if (h == 2) {
                se.first += 1;
                n_held += 1;
            }
        }
    }
    float min_cov = INFINITY, max_cov = -INFINITY;
    size_t well = 0;
    for (const auto &kv : seq_stats) {
        const float c = (float)kv.second.first / (float)kv.second.second * 100.0f;
        min_cov = std::fmin(min_cov, c);
        max_cov = std::fmax(max_cov, c);
        if (c >= 80.0f) ++well;
    }
    size_t idle = 0;
    for (size_t i = 0; i < n_primers; ++i)
        if (!primer_held[i]) ++idle;
    std::string out = std::string("\nCoverage report (thal ") + (mode == 2 ? "END1" : "ANY") + ", t >= " +
                      fmt("%.2f", (double)tm_threshold) + " C; matches within " + std::to_string(max_mismatches) +
                      " mismatches, last " + std::to_string(exact_3p) + " bases exact):\n";
    out += "  Segments:  " + std::to_string(n_held) + "/" + std::to_string(total) + " held (" +
           fmt("%.1f", (double)(100.0f * (float)n_held / (float)total)) + "%), " + std::to_string(matched) + "/" +
           std::to_string(total) + " matched\n";
    out += "  Sequences: " + std::to_string(well) + "/" + std::to_string(seq_stats.size()) +
           " at \xe2\x89\xa5" "80% held (min " + fmt("%.1f", (double)min_cov) + "%, max " +
           fmt("%.1f", (double)max_cov) + "%)\n";
    out += "  Primers:   " + std::to_string(idle) + " of " + std::to_string(n_primers) + " hold no segment\n";
    return out;
}

std::string coverage_report_thal(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                                 const std::vector<KmerStat> &rev, const std::vector<SequenceRecord> &records,
                                 int segment_size, int overlap_size, int window_size, int kmer_size, int max_mismatches,
                                 int exact_3p, const msspe_chem &chem, int mode, float tm_threshold)
{
    const size_t L = aln.length();
    const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
    std::vector<uint8_t> held(records.size() * P + 1, 0);
    std::vector<uint32_t> primer_held(fwd.size() + rev.size() + 1, 0);
    if (P) {
        const auto wf = pack_words(eng, fwd, kmer_size), wr = pack_words(eng, rev, kmer_size);
        const msspe_kmer_opt opt{segment_size, overlap_size, window_size, kmer_size, 0, 0};
        const msspe_mismatch_opt mm{max_mismatches, exact_3p};
        const int rc = msspe_segment_coverage_thal_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm,
                                                              wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                              &chem, mode, tm_threshold, held.data(), nullptr, nullptr,
                                                              primer_held.data(), nullptr, 0, nullptr);
        if (rc) eng.fail(rc);
    }
    return coverage_thal_block(records, P, segment_size, overlap_size, held.data(), primer_held.data(),
                               fwd.size() + rev.size(), max_mismatches, exact_3p, mode, tm_threshold);
}

std::string seed_report(int max_mismatches, int exact_3p, int mode, float tm_threshold, size_t covered_f, size_t panel_f,
                        size_t covered_r, size_t panel_r, size_t segments)
{
    std::string s = "\nSeeding (up to " + std::to_string(max_mismatches) + " mismatches, last " + std::to_string(exact_3p) +
                    " bases exact";
    if (mode) s += std::string("; thal ") + (mode == 2 ? "END1" : "ANY") + ", t >= " + fmt("%.2f", (double)tm_threshold) + " C";
    const std::string t = std::to_string(segments);
    return s + "):\n  Forward: " + std::to_string(covered_f) + " of " + t + " segments covered by " +
           std::to_string(panel_f) + " panel primers; Reverse: " + std::to_string(covered_r) + " of " + t +
           " segments covered by " + std::to_string(panel_r) + " panel primers\n";
}

std::string thin_thal_report(int mode, float tm_threshold, int max_mismatches, int exact_3p, int min_gain,
                             size_t kept_f, size_t n_f, size_t kept_r, size_t n_r, size_t forced, size_t held_all,
                             size_t held_kept, size_t segments, int depth, size_t deep_all, size_t deep_kept)
{
    const std::string x = std::to_string(kept_f + kept_r), y = std::to_string(n_f + n_r), t = std::to_string(segments);
    return std::string("\nPanel thinning (thal ") + (mode == 2 ? "END1" : "ANY") + ", t >= " +
           fmt("%.2f", (double)tm_threshold) + " C; matches within " + std::to_string(max_mismatches) +
           " mismatches, last " + std::to_string(exact_3p) + " bases exact, gain >= " + std::to_string(min_gain) +
           thin_depth_tag(depth) +
           "):\n  Primers:  kept " + x + " of " + y + " (forward " + std::to_string(kept_f) + " of " +
           std::to_string(n_f) + ", reverse " + std::to_string(kept_r) + " of " + std::to_string(n_r) + "), " +
           std::to_string(forced) + " forced\n  Segments: held " + std::to_string(held_all) + "/" + t + " by all " + y +
           ", " + std::to_string(held_kept) + "/" + t + " by the kept " + x + "\n" +
           thin_depth_line(depth, deep_all, deep_kept, t, y, x);
}

std::string thin_panel_on_device(Engine &eng, const DeviceAlignment &aln, std::vector<KmerStat> &fwd,
                                 std::vector<KmerStat> &rev, const std::vector<std::string> &panel_f,
                                 const std::vector<std::string> &panel_r, int segment_size, int overlap_size,
                                 int window_size, int kmer_size, int max_mismatches, int exact_3p, int min_gain,
                                 const msspe_chem *chem, int mode, float tm_threshold, int depth,
                                 const std::vector<uint32_t> *genome_weights, const PrimerCostFn *costs)
{
    // the new primers in their lists' order (stage A's selection order: ties go to the word with more postings), the
    // panel's behind them, forced
    std::vector<KmerStat> all_f = fwd, all_r = rev;
    for (const auto &w : panel_f) all_f.push_back(KmerStat{w, SEQ_DIR_FWD});
    for (const auto &w : panel_r) all_r.push_back(KmerStat{w, SEQ_DIR_REV});
    const size_t n = all_f.size() + all_r.size();
    std::vector<uint8_t> forced(n + 1, 0), keep(n + 1, 0);
    for (size_t i = fwd.size(); i < all_f.size(); ++i) forced[i] = 1;
    for (size_t i = rev.size(); i < all_r.size(); ++i) forced[all_f.size() + i] = 1;
    std::vector<uint32_t> order(n + 1), gains(n + 1);
    int n_picked = 0;
    long long covered_all = 0, covered_kept = 0;
    const size_t L = aln.length();
    const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
    const auto wf = pack_words(eng, all_f, kmer_size), wr = pack_words(eng, all_r, kmer_size);
    const msspe_kmer_opt opt{segment_size, overlap_size, window_size, kmer_size, 0, 0};
    const msspe_mismatch_opt mm{max_mismatches, exact_3p};
    const msspe_thin_opt thin{min_gain};
    const msspe_thin_depth_opt deep{min_gain, depth};
    long long counts[4] = {0, 0, 0, 0};   // depth above 1: covered_all / covered_kept are counts[0] / [1]
    std::vector<uint32_t> weights;   // --genome-weights: every segment of a row weighs what its genome weighs
    uint64_t weight_all = 0, weight_kept = 0, weight_total = 0;
    if (genome_weights)
        for (const uint32_t w : *genome_weights) weights.insert(weights.end(), P, w), weight_total += (uint64_t)w * P;
    std::vector<uint32_t> cost;   // --primer-costs / --background-site-cost: the lists' primers, then the panel's
    uint64_t cost_all = 0, cost_kept = 0;
    if (costs) {
        std::vector<std::string> words;
        for (const auto *list : {&all_f, &all_r})
            for (const auto &s : *list) words.push_back(s.word);
        cost = (*costs)(words);
    }
    const int rc =
        costs   // (depth 1, no chemistry: Args::parse refuses the rest); with the weights when given
            ? msspe_panel_thin_cost_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &thin, wf.data(),
                                               (int)wf.size(), wr.data(), (int)wr.size(), forced.data(),
                                               genome_weights ? weights.data() : nullptr, cost.data(), keep.data(),
                                               order.data(), gains.data(), &n_picked, nullptr, &covered_all,
                                               &covered_kept, &weight_all, &weight_kept, &cost_all, &cost_kept)
        : genome_weights   // (depth 1, no chemistry: Args::parse refuses the rest)
            ? msspe_panel_thin_weighted_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &thin, wf.data(),
                                                   (int)wf.size(), wr.data(), (int)wr.size(), forced.data(),
                                                   weights.data(), keep.data(), order.data(), gains.data(), &n_picked,
                                                   nullptr, &covered_all, &covered_kept, &weight_all, &weight_kept)
        : depth > 1
            ? (chem ? msspe_panel_thin_thal_depth_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &deep,
                                                             chem, mode, tm_threshold, wf.data(), (int)wf.size(),
                                                             wr.data(), (int)wr.size(), forced.data(), keep.data(),
                                                             order.data(), gains.data(), &n_picked, nullptr, nullptr,
                                                             counts)
                    : msspe_panel_thin_depth_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &deep,
                                                        wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                        forced.data(), keep.data(), order.data(), gains.data(),
                                                        &n_picked, nullptr, nullptr, counts))
        : chem ? msspe_panel_thin_thal_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &thin, chem, mode,
                                                tm_threshold, wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                forced.data(), keep.data(), order.data(), gains.data(), &n_picked,
                                                nullptr, &covered_all, &covered_kept)
             : msspe_panel_thin_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &mm, &thin, wf.data(),
                                           (int)wf.size(), wr.data(), (int)wr.size(), forced.data(), keep.data(),
                                           order.data(), gains.data(), &n_picked, nullptr, &covered_all,
                                           &covered_kept);
    if (rc) eng.fail(rc);
    if (depth > 1) {
        covered_all = counts[0];
        covered_kept = counts[1];
    }
    const size_t n_f = fwd.size(), n_r = rev.size();
    std::vector<KmerStat> kept_f, kept_r;
    for (size_t i = 0; i < n_f; ++i)
        if (keep[i]) kept_f.push_back(fwd[i]);
    for (size_t i = 0; i < n_r; ++i)
        if (keep[all_f.size() + i]) kept_r.push_back(rev[i]);
    fwd.swap(kept_f);
    rev.swap(kept_r);
    if (chem)
        return thin_thal_report(mode, tm_threshold, max_mismatches, exact_3p, min_gain, fwd.size(), n_f, rev.size(),
                                n_r, panel_f.size() + panel_r.size(), (size_t)covered_all, (size_t)covered_kept,
                                (size_t)aln.rows() * P, depth, (size_t)counts[2], (size_t)counts[3]);
    const std::string block = thin_report(max_mismatches, exact_3p, min_gain, fwd.size(), n_f, rev.size(), n_r,
                                          panel_f.size() + panel_r.size(), (size_t)covered_all, (size_t)covered_kept,
                                          (size_t)aln.rows() * P, depth, (size_t)counts[2], (size_t)counts[3]);
    std::string lines;   // behind "Segments:": the weights' line, then the costs'
    if (genome_weights) lines += weight_line(weight_all, weight_kept, weight_total, n_f + n_r, fwd.size() + rev.size());
    if (costs) lines += cost_line(cost_kept, cost_all, fwd.size() + rev.size() + panel_f.size() + panel_r.size(), n);
    return lines.empty() ? block : with_weight_line(block, lines);
}

std::string select_report(int mode, float tm_threshold, int max_mismatches, int exact_3p, int min_gain, int max_tubes,
                          size_t kept_f, size_t n_f, size_t kept_r, size_t n_r, size_t forced, size_t barred,
                          size_t covered_all, size_t covered_kept, size_t segments, const std::vector<size_t> *per_tube,
                          int depth, size_t deep_all, size_t deep_kept)
{
    const std::string x = std::to_string(kept_f + kept_r), y = std::to_string(n_f + n_r), t = std::to_string(segments);
    const std::string what = mode ? "held " : "covered ";
    std::string s = "\nPanel selection by coverage (";
    if (mode)
        s += std::string("thal ") + (mode == 2 ? "END1" : "ANY") + ", t >= " + fmt("%.2f", (double)tm_threshold) +
             " C; matches within " + std::to_string(max_mismatches) + " mismatches, last ";
    else
        s += "up to " + std::to_string(max_mismatches) + " mismatches, last ";
    s += std::to_string(exact_3p) + " bases exact, gain >= " + std::to_string(min_gain) + ", tubes <= " +
         std::to_string(max_tubes) + thin_depth_tag(depth) + "):\n  Rule:     each round keeps the primer with the most new segments and bars its "
         "conflict neighbours from its tube\n  Primers:  kept " + x + " of " + y + " (forward " + std::to_string(kept_f) +
         " of " + std::to_string(n_f) + ", reverse " + std::to_string(kept_r) + " of " + std::to_string(n_r) + "), " +
         std::to_string(forced) + " forced\n  Barred:   " + std::to_string(barred) + " by conflicts\n  Segments: " + what +
         std::to_string(covered_all) + "/" + t + " by all " + y + ", " + std::to_string(covered_kept) + "/" + t +
         " by the kept " + x + "\n" + thin_depth_line(depth, deep_all, deep_kept, t, y, x);
    if (per_tube)
        for (size_t i = 0; i < per_tube->size(); ++i)
            s += "  Tube " + std::to_string(i + 1) + ": " + std::to_string((*per_tube)[i]) + " primers\n";
    return s;
}

std::string select_panel_on_device(Engine &eng, const DeviceAlignment &aln, const std::vector<KmerStat> &fwd,
                                   const std::vector<KmerStat> &rev, const std::vector<std::string> &panel_f,
                                   const std::vector<std::string> &panel_r, int segment_size, int overlap_size,
                                   int window_size, int kmer_size, int max_mismatches, int exact_3p, int min_gain,
                                   const msspe_chem &chem, int mode, float tm_threshold, int max_tubes, bool list_tubes,
                                   bool screen, bool drop_self_pairs, float dg_threshold, std::vector<KmerStat> &kept_f,
                                   std::vector<KmerStat> &kept_r, std::map<std::string, int> &tubes,
                                   const std::function<void(const KmerStat &, bool)> &dropped,
                                   const NtthalOptions *end_rule, int depth,
                                   const std::vector<uint32_t> *genome_weights, const PrimerCostFn *costs)
{
    // the graph's nodes are distinct words: the panel's first, then the new primers in their lists' order; a word met
    // again (the other direction's list) is not offered
    std::unordered_set<std::string> seen;
    std::vector<KmerStat> all_f, all_r;
    std::vector<size_t> src_f, src_r;   // the offered primers' places in fwd / rev
    std::vector<char> offered_f(fwd.size(), 0), offered_r(rev.size(), 0);
    for (const auto *panel : {&panel_f, &panel_r})
        for (const auto &w : *panel) seen.insert(w);
    for (size_t i = 0; i < fwd.size(); ++i)
        if (seen.insert(fwd[i].word).second) all_f.push_back(fwd[i]), src_f.push_back(i), offered_f[i] = 1;
    for (size_t i = 0; i < rev.size(); ++i)
        if (seen.insert(rev[i].word).second) all_r.push_back(rev[i]), src_r.push_back(i), offered_r[i] = 1;
    const size_t new_f = all_f.size(), new_r = all_r.size();
    seen.clear();
    for (const auto &w : panel_f)
        if (seen.insert(w).second) all_f.push_back(KmerStat{w, SEQ_DIR_FWD});
    for (const auto &w : panel_r)
        if (seen.insert(w).second) all_r.push_back(KmerStat{w, SEQ_DIR_REV});
    const size_t n = all_f.size() + all_r.size(), W = (n + 63) / 64;
    std::vector<uint8_t> forced(n + 1, 0), keep(n + 1, 0), tube(n + 1, MSSPE_TUBE_NONE), barred(n + 1, 0);
    for (size_t i = new_f; i < all_f.size(); ++i) forced[i] = 1;
    for (size_t i = new_r; i < all_r.size(); ++i) forced[all_f.size() + i] = 1;
    std::vector<uint32_t> order(n + 1), gains(n + 1);
    int n_picked = 0, used = 0;
    long long covered_all = 0, covered_kept = 0, counts[4] = {0, 0, 0, 0};   // counts: --select-depth above 1
    const size_t L = aln.length();
    const size_t P = L < (size_t)segment_size ? 0 : (L - (size_t)segment_size) / (size_t)overlap_size + 1;
    const auto wf = pack_words(eng, all_f, kmer_size), wr = pack_words(eng, all_r, kmer_size);
    void *d_pool = nullptr, *d_bitmap = nullptr;
    std::vector<uint32_t> weights;   // --genome-weights: every segment of a row weighs what its genome weighs
    uint64_t weight_all = 0, weight_kept = 0, weight_total = 0;
    std::vector<uint32_t> cost;
    uint64_t cost_all = 0, cost_kept = 0;
    int rc = MSSPE_OK;
    if (n) {
        const std::vector<uint64_t> zero(n * W, 0);
        rc = msspe_device_put(eng.ctx(), zero.data(), sizeof(uint64_t) * zero.size(), &d_bitmap);
        if (!rc && screen) {   // --check-cross-dimers false: no edges at all
            std::vector<uint64_t> pool(wf);
            pool.insert(pool.end(), wr.begin(), wr.end());
            rc = msspe_device_put(eng.ctx(), pool.data(), sizeof(uint64_t) * n, &d_pool);
            // the screen's decisions only: the bitmap is all the selection reads
            if (!rc && end_rule && end_rule->use_end) {   // --max-cross-dimer-end-tm: the union, and its kinds for stdout
                const msspe_conflict_rule both = conflict_rule(*end_rule);
                const uint64_t zero3[3] = {0, 0, 0};
                uint64_t kinds[3] = {0, 0, 0};
                void *d_kinds = nullptr;
                rc = msspe_device_put(eng.ctx(), zero3, sizeof zero3, &d_kinds);
                if (!rc)
                    rc = msspe_conflict_graph_dev(eng.ctx(), static_cast<const uint64_t *>(d_pool), (int)n, kmer_size, &chem,
                                                  &both, 0, (int)n, 0, (int)n, nullptr, static_cast<uint64_t *>(d_bitmap),
                                                  static_cast<uint64_t *>(d_kinds));
                if (!rc) rc = msspe_synchronize(eng.ctx());
                if (!rc) rc = msspe_device_get(eng.ctx(), d_kinds, sizeof kinds, kinds);
                if (d_kinds) (void)msspe_device_free(eng.ctx(), d_kinds);
                if (!rc) note_kinds(*end_rule, n, kinds);
            } else if (!rc)
                rc = msspe_cross_dimer_dev(eng.ctx(), static_cast<const uint64_t *>(d_pool), (int)n, kmer_size, &chem,
                                           dg_threshold, 0, (int)n, 0, (int)n, nullptr,
                                           static_cast<uint64_t *>(d_bitmap), nullptr, nullptr);
            if (!rc) rc = msspe_synchronize(eng.ctx());   // (and the hand-over lists held)
        }
    }
    if (!rc) {
        const msspe_kmer_opt opt{segment_size, overlap_size, window_size, kmer_size, 0, 0};
        const msspe_seed_rule rule{max_mismatches, exact_3p, mode, mode ? &chem : nullptr, tm_threshold};
        const msspe_select_opt so{min_gain, max_tubes, drop_self_pairs ? 1 : 0};
        const msspe_select_depth_opt deep{min_gain, max_tubes, drop_self_pairs ? 1 : 0, depth};
        if (genome_weights)
            for (const uint32_t w : *genome_weights) weights.insert(weights.end(), P, w), weight_total += (uint64_t)w * P;
        if (costs) {   // --primer-costs / --background-site-cost: the offered primers, then the panel's
            std::vector<std::string> words;
            for (const auto *list : {&all_f, &all_r})
                for (const auto &s : *list) words.push_back(s.word);
            cost = (*costs)(words);
        }
        rc = costs   // (depth 1: Args::parse refuses the rest); with the weights when given
                 ? msspe_panel_select_cost_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &rule, &so,
                                                      wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                      forced.data(), static_cast<const uint64_t *>(d_bitmap),
                                                      genome_weights ? weights.data() : nullptr, cost.data(),
                                                      keep.data(), order.data(), gains.data(), &n_picked, tube.data(),
                                                      barred.data(), nullptr, &covered_all, &covered_kept, &used,
                                                      &weight_all, &weight_kept, &cost_all, &cost_kept)
             : genome_weights   // (depth 1: Args::parse refuses the rest)
                 ? msspe_panel_select_weighted_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &rule, &so,
                                                          wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                          forced.data(), static_cast<const uint64_t *>(d_bitmap),
                                                          weights.data(), keep.data(), order.data(), gains.data(),
                                                          &n_picked, tube.data(), barred.data(), nullptr, &covered_all,
                                                          &covered_kept, &used, &weight_all, &weight_kept)
             : depth <= 1
                 ? msspe_panel_select_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &rule, &so, wf.data(),
                                                 (int)wf.size(), wr.data(), (int)wr.size(), forced.data(),
                                                 static_cast<const uint64_t *>(d_bitmap), keep.data(), order.data(),
                                                 gains.data(), &n_picked, tube.data(), barred.data(), nullptr,
                                                 &covered_all, &covered_kept, &used)
                 : msspe_panel_select_depth_packed_dev(eng.ctx(), aln.device(), aln.rows(), L, &opt, &rule, &deep,
                                                       wf.data(), (int)wf.size(), wr.data(), (int)wr.size(),
                                                       forced.data(), static_cast<const uint64_t *>(d_bitmap),
                                                       keep.data(), order.data(), gains.data(), &n_picked, tube.data(),
                                                       barred.data(), &used, nullptr, nullptr, nullptr, counts);
        if (depth > 1) covered_all = counts[0], covered_kept = counts[1];
    }
    if (d_pool) (void)msspe_device_free(eng.ctx(), d_pool);
    if (d_bitmap) (void)msspe_device_free(eng.ctx(), d_bitmap);
    if (rc) eng.fail(rc);
    std::vector<size_t> per_tube((size_t)used, 0);
    std::vector<char> kept_of_f(fwd.size(), 0), kept_of_r(rev.size(), 0), barred_f(fwd.size(), 0), barred_r(rev.size(), 0);
    size_t n_barred = 0;
    for (size_t i = 0; i < new_f + new_r; ++i) {
        const bool f = i < new_f;
        const size_t at = f ? i : all_f.size() + (i - new_f), src = f ? src_f[i] : src_r[i - new_f];
        (f ? kept_of_f : kept_of_r)[src] = (char)keep[at];
        (f ? barred_f : barred_r)[src] = (char)barred[at];
        n_barred += barred[at];
        if (keep[at]) {
            tubes[(f ? fwd : rev)[src].word] = tube[at];
            if (tube[at] < per_tube.size()) ++per_tube[tube[at]];
        }
    }
    for (size_t i = 0; i < fwd.size(); ++i)
        if (kept_of_f[i]) kept_f.push_back(fwd[i]);
        else dropped(fwd[i], barred_f[i] != 0);
    for (size_t i = 0; i < rev.size(); ++i)
        if (kept_of_r[i]) kept_r.push_back(rev[i]);
        else dropped(rev[i], barred_r[i] != 0);
    const std::string block =
        select_report(mode, tm_threshold, max_mismatches, exact_3p, min_gain, max_tubes, kept_f.size(), fwd.size(),
                      kept_r.size(), rev.size(), n - new_f - new_r, n_barred, (size_t)covered_all, (size_t)covered_kept,
                      (size_t)aln.rows() * P, list_tubes ? &per_tube : nullptr, depth, (size_t)counts[2],
                      (size_t)counts[3]);
    std::string lines;   // behind "Segments:": the weights' line, then the costs'
    if (genome_weights)
        lines += weight_line(weight_all, weight_kept, weight_total, fwd.size() + rev.size(),
                             kept_f.size() + kept_r.size());
    if (costs) {
        size_t n_kept = 0;
        for (size_t p = 0; p < n; ++p) n_kept += keep[p];
        lines += cost_line(cost_kept, cost_all, n_kept, n);
    }
    return lines.empty() ? block : with_weight_line(block, lines);
}

DeviceBackground::DeviceBackground(Engine &eng, const std::vector<SequenceRecord> &records)
    : eng_(eng), names_(records.size()), starts_(records.size())
{
    std::vector<const char *> rows(records.size());
    std::vector<size_t> bytes(records.size());
    for (size_t r = 0; r < records.size(); ++r) {
        rows[r] = records[r].sequence.data();
        bytes[r] = records[r].sequence.size();
        names_[r] = records[r].name;
    }
    const int rc = msspe_device_put_stream_packed(eng.ctx(), rows.data(), bytes.data(), (int)records.size(), &dev_,
                                                  &len_, starts_.data());
    if (rc) eng.fail(rc);
}

DeviceBackground::~DeviceBackground()
{
    if (dev_) (void)msspe_device_free(eng_.ctx(), dev_);
}

std::vector<std::pair<uint64_t, uint64_t>> DeviceBackground::sites(const std::vector<std::string> &words,
                                                                  int max_mismatches, int exact_3p) const
{
    std::vector<std::pair<uint64_t, uint64_t>> out(words.size());
    std::map<size_t, std::vector<size_t>> by_length;   // a panel of mixed lengths: one length class per call
    for (size_t i = 0; i < words.size(); ++i) by_length[words[i].size()].push_back(i);
    for (const auto &cls : by_length) {
        const int k = (int)cls.first, n = (int)cls.second.size();
        std::string flat;
        for (const size_t i : cls.second) flat += words[i];
        std::vector<uint64_t> packed((size_t)n), counts(2 * (size_t)n);
        int rc = msspe_pack_oligos(flat.data(), n, k, packed.data());
        if (rc) eng_.fail(rc);
        const msspe_mismatch_opt mm{std::min(max_mismatches, k), std::min(exact_3p, k)};
        rc = msspe_background_sites_packed_dev(eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm,
                                               packed.data(), n, counts.data(), nullptr, 0, nullptr);
        if (rc) eng_.fail(rc);
        for (int j = 0; j < n; ++j) out[cls.second[(size_t)j]] = {counts[2 * (size_t)j], counts[2 * (size_t)j + 1]};
    }
    return out;
}

std::vector<std::pair<uint64_t, uint64_t>> DeviceBackground::scored(
    const std::vector<std::string> &words, int max_mismatches, int exact_3p, const msspe_chem &chem, int mode,
    float tm_threshold, std::vector<std::pair<uint64_t, uint64_t>> &stable_out, int flank) const
{
    std::vector<std::pair<uint64_t, uint64_t>> out(words.size());
    stable_out.assign(words.size(), {0, 0});
    std::map<size_t, std::vector<size_t>> by_length;   // a panel of mixed lengths: one length class per call
    for (size_t i = 0; i < words.size(); ++i) by_length[words[i].size()].push_back(i);
    for (const auto &cls : by_length) {
        const int k = (int)cls.first, n = (int)cls.second.size();
        std::string flat;
        for (const size_t i : cls.second) flat += words[i];
        std::vector<uint64_t> packed((size_t)n), counts(2 * (size_t)n), stable(2 * (size_t)n);
        int rc = msspe_pack_oligos(flat.data(), n, k, packed.data());
        if (rc) eng_.fail(rc);
        const msspe_mismatch_opt mm{std::min(max_mismatches, k), std::min(exact_3p, k)};
        const int f = std::min(flank, std::max(0, (32 - k) / 2));
        rc = f ? msspe_background_thal_flank_packed_dev(eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm,
                                                        packed.data(), n, &chem, mode, tm_threshold, f, counts.data(),
                                                        stable.data(), nullptr, 0, nullptr)
               : msspe_background_thal_packed_dev(eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm,
                                                  packed.data(), n, &chem, mode, tm_threshold, counts.data(),
                                                  stable.data(), nullptr, 0, nullptr);
        if (rc) eng_.fail(rc);
        for (int j = 0; j < n; ++j) {
            out[cls.second[(size_t)j]] = {counts[2 * (size_t)j], counts[2 * (size_t)j + 1]};
            stable_out[cls.second[(size_t)j]] = {stable[2 * (size_t)j], stable[2 * (size_t)j + 1]};
        }
    }
    return out;
}

std::vector<std::pair<uint64_t, uint64_t>> DeviceBackground::amplicons(
    const std::vector<std::string> &words, int max_mismatches, int exact_3p, const msspe_chem &chem, int mode,
    float tm_threshold, uint32_t min_len, uint32_t max_len, std::vector<std::pair<uint64_t, uint64_t>> &stable_out,
    std::vector<std::pair<uint64_t, uint64_t>> &amplicons_out, std::vector<msspe_amplicon> &list_out,
    int flank) const
{
    std::vector<std::pair<uint64_t, uint64_t>> out(words.size());
    stable_out.assign(words.size(), {0, 0});
    amplicons_out.assign(words.size(), {0, 0});
    list_out.clear();
    std::map<size_t, std::vector<size_t>> by_length;   // a panel of mixed lengths: one length class per call
    for (size_t i = 0; i < words.size(); ++i) by_length[words[i].size()].push_back(i);
    for (const auto &cls : by_length) {
        const int k = (int)cls.first, n = (int)cls.second.size();
        std::string flat;
        for (const size_t i : cls.second) flat += words[i];
        std::vector<uint64_t> packed((size_t)n), counts(2 * (size_t)n), stable(2 * (size_t)n), amps(2 * (size_t)n);
        int rc = msspe_pack_oligos(flat.data(), n, k, packed.data());
        if (rc) eng_.fail(rc);
        const msspe_mismatch_opt mm{std::min(max_mismatches, k), std::min(exact_3p, k)};
        // primers longer than max_len make no product that short: the scored counts alone
        const bool pair = (uint32_t)k <= max_len;
        const msspe_amplicon_opt opt{pair ? std::max(min_len, (uint32_t)k) : (uint32_t)k, pair ? max_len : (uint32_t)k};
        uint64_t total = 0, count = 0;
        std::vector<msspe_amplicon> list;
        // the device list with its count behind it; a list that was too short says how long it must be
        for (uint64_t capacity = (uint64_t)1 << 16;; capacity = count) {
            const size_t list_bytes = sizeof(msspe_amplicon) * (size_t)capacity;
            const std::vector<char> zero(list_bytes + sizeof(uint64_t), 0);
            void *d_list = nullptr;
            if ((rc = msspe_device_put(eng_.ctx(), zero.data(), zero.size(), &d_list))) eng_.fail(rc);
            uint64_t *d_count = reinterpret_cast<uint64_t *>(static_cast<char *>(d_list) + list_bytes);
            const int f = std::min(flank, std::max(0, (32 - k) / 2));
            msspe_amplicon *d_amps = pair ? static_cast<msspe_amplicon *>(d_list) : nullptr;
            rc = f ? msspe_background_amplicons_flank_packed_dev(
                         eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm, packed.data(), n, &chem, mode,
                         tm_threshold, f, &opt, starts_.data(), (int)starts_.size(), counts.data(), stable.data(),
                         amps.data(), &total, d_amps, capacity, d_count)
                   : msspe_background_amplicons_packed_dev(
                         eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm, packed.data(), n, &chem, mode,
                         tm_threshold, &opt, starts_.data(), (int)starts_.size(), counts.data(), stable.data(),
                         amps.data(), &total, d_amps, capacity, d_count);
            if (!rc) rc = msspe_device_get(eng_.ctx(), d_count, sizeof count, &count);
            if (!rc && count <= capacity) {
                list.resize((size_t)count);
                rc = msspe_device_get(eng_.ctx(), d_list, sizeof(msspe_amplicon) * list.size(), list.data());
            }
            (void)msspe_device_free(eng_.ctx(), d_list);
            if (rc) eng_.fail(rc);
            if (count <= capacity) break;
        }
        for (int j = 0; j < n; ++j) {
            const size_t i = cls.second[(size_t)j];
            out[i] = {counts[2 * (size_t)j], counts[2 * (size_t)j + 1]};
            stable_out[i] = {stable[2 * (size_t)j], stable[2 * (size_t)j + 1]};
            if (pair) amplicons_out[i] = {amps[2 * (size_t)j], amps[2 * (size_t)j + 1]};
        }
        for (msspe_amplicon a : list) {
            a.fwd = (uint32_t)cls.second[a.fwd];
            a.rev = (uint32_t)cls.second[a.rev];
            list_out.push_back(a);
        }
    }
    std::sort(list_out.begin(), list_out.end(), [](const msspe_amplicon &a, const msspe_amplicon &b) {
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.len != b.len) return a.len < b.len;
        if (a.fwd != b.fwd) return a.fwd < b.fwd;
        return a.rev < b.rev;
    });
    return out;
}

std::pair<std::string, uint64_t> DeviceBackground::locate(uint64_t pos) const
{
    const size_t r = (size_t)(std::upper_bound(starts_.begin(), starts_.end(), pos) - starts_.begin()) - 1;
    return {names_[r], pos - starts_[r]};
}

std::string background_report_amplicons(const std::vector<std::string> &names,
                                        const std::vector<std::pair<uint64_t, uint64_t>> &counts,
                                        const std::vector<msspe_amplicon> &list, const DeviceBackground &background,
                                        uint32_t min_len, uint32_t max_len)
{
    std::string out = "\nBackground amplicons (stable sites facing each other, " + std::to_string(min_len) + " to " +
                      std::to_string(max_len) + " bases):\n";
    uint64_t total = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        out += "  " + names[i] + ": as forward " + std::to_string(counts[i].first) + ", as reverse " +
               std::to_string(counts[i].second) + "\n";
        total += counts[i].first;
    }
    out += "  Total: " + std::to_string(names.size()) + " primers, " + std::to_string(total) + " amplicons\n";
    const size_t shown = std::min<size_t>(20, list.size());
    out += "  First " + std::to_string(shown) + " (record:offset, length, forward, reverse):\n";
    for (size_t e = 0; e < shown; ++e) {
        const auto at = background.locate(list[e].pos);
        out += "    " + at.first + ":" + std::to_string(at.second) + ", " + std::to_string(list[e].len) + ", " +
               names[list[e].fwd] + ", " + names[list[e].rev] + "\n";
    }
    return out;
}

std::vector<msspe_reach_record> target_reach(Engine &eng, const std::vector<SequenceRecord> &records,
                                             const std::vector<std::string> &words, int k, int max_mismatches,
                                             int exact_3p, const msspe_chem &chem, int mode, float tm_threshold,
                                             uint32_t reach, std::vector<std::string> &genomes_out,
                                             ReachThinning *thin)
{
    if (thin) {
        thin->keep = thin->forced;
        thin->reached_all = thin->reached_kept = 0;
    }
    for (const auto &w : words)
        if ((int)w.size() != k)
            throw std::runtime_error("--reach needs primers of one length, --kmer-size " + std::to_string(k) +
                                     ": '" + w + "' has " + std::to_string(w.size()) + " bases");
    std::vector<SequenceRecord> rows(records.size());   // each input row without its gap columns
    genomes_out.assign(records.size(), std::string());
    for (size_t r = 0; r < records.size(); ++r) {
        rows[r].name = records[r].name;
        for (const char c : records[r].sequence)
            if (c != '-') rows[r].sequence.push_back(c);
        genomes_out[r] = rows[r].sequence;
    }
    std::vector<msspe_reach_record> out(records.size());
    if (records.empty()) return out;
    DeviceBackground stream(eng, rows);   // uploaded once, freed when the report is done
    const int n = (int)words.size();
    std::string flat;
    for (const auto &w : words) flat += w;
    std::vector<uint64_t> packed((size_t)std::max(n, 1)), counts(2 * (size_t)std::max(n, 1)),
        stable(2 * (size_t)std::max(n, 1));
    int rc = n ? msspe_pack_oligos(flat.data(), n, k, packed.data()) : 0;
    if (rc) eng.fail(rc);
    const msspe_mismatch_opt mm{std::min(max_mismatches, k), std::min(exact_3p, k)};
    const msspe_reach_opt opt{reach};
    if (thin) {
        std::vector<uint32_t> order((size_t)std::max(n, 1)), gains((size_t)std::max(n, 1));
        int n_picked = 0;
        thin->forced.resize((size_t)std::max(n, 1), 0);
        thin->keep.assign((size_t)std::max(n, 1), 0);
        rc = stream.thin_reach(k, mm, packed, n, chem, mode, tm_threshold, opt, thin->min_gain, thin->forced,
                               thin->keep, order, gains, n_picked, thin->reached_all, thin->reached_kept, counts,
                               stable, out);
        thin->forced.resize((size_t)n);
        thin->keep.resize((size_t)n);
    } else {
        rc = stream.reach(k, mm, packed, n, chem, mode, tm_threshold, opt, counts, stable, out);
    }
    if (rc) eng.fail(rc);
    return out;
}

int DeviceBackground::thin_reach(int k, const msspe_mismatch_opt &mm, const std::vector<uint64_t> &packed, int n,
                                 const msspe_chem &chem, int mode, float tm_threshold, const msspe_reach_opt &opt,
                                 int min_gain, const std::vector<uint8_t> &forced, std::vector<uint8_t> &keep,
                                 std::vector<uint32_t> &order, std::vector<uint32_t> &gains, int &n_picked,
                                 long long &reached_all, long long &reached_kept, std::vector<uint64_t> &counts,
                                 std::vector<uint64_t> &stable, std::vector<msspe_reach_record> &out) const
{
    const msspe_thin_opt thin{min_gain};
    return msspe_panel_thin_reach_packed_dev(eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm,
                                             packed.data(), n, &chem, mode, tm_threshold, 0, &opt, &thin,
                                             forced.data(), starts_.data(), (int)starts_.size(), keep.data(),
                                             order.data(), gains.data(), &n_picked, nullptr, &reached_all,
                                             &reached_kept, counts.data(), stable.data(), out.data());
}

int DeviceBackground::reach(int k, const msspe_mismatch_opt &mm, const std::vector<uint64_t> &packed, int n,
                            const msspe_chem &chem, int mode, float tm_threshold, const msspe_reach_opt &opt,
                            std::vector<uint64_t> &counts, std::vector<uint64_t> &stable,
                            std::vector<msspe_reach_record> &out) const
{
    return msspe_stream_reach_packed_dev(eng_.ctx(), static_cast<const uint64_t *>(dev_), len_, k, &mm, packed.data(),
                                         n, &chem, mode, tm_threshold, 0, &opt, starts_.data(), (int)starts_.size(),
                                         counts.data(), stable.data(), out.data());
}

static std::string reach_rule(int max_mismatches, int exact_3p, bool scored, int mode, float tm_threshold)
{
    std::string out = "up to " + std::to_string(max_mismatches) + " mismatches, last " + std::to_string(exact_3p) +
                      " bases exact";
    if (scored) {
        char thr[64];
        std::snprintf(thr, sizeof thr, "%.2f", (double)tm_threshold);
        out += std::string("; stable: thal ") + (mode == 2 ? "END1" : "ANY") + " t >= " + thr + " C";
    }
    return out;
}

std::string reach_thinning_report(const ReachThinning &thin, uint32_t reach, int max_mismatches, int exact_3p,
                                  bool scored, int mode, float tm_threshold)
{
    size_t kept = 0, forced = 0;
    for (const uint8_t f : thin.keep) kept += f != 0;
    for (const uint8_t f : thin.forced) forced += f != 0;
    std::string out = "\nReach thinning (extension " + std::to_string(reach) + " bases, min gain " +
                      std::to_string(thin.min_gain) + "; sites: " +
                      reach_rule(max_mismatches, exact_3p, scored, mode, tm_threshold) + "):\n";
    out += "  Kept " + std::to_string(kept) + " of " + std::to_string(thin.keep.size()) + " primers (" +
           std::to_string(forced) + " forced)\n";
    out += "  Columns reached by all: " + std::to_string(thin.reached_all) + ", by kept: " +
           std::to_string(thin.reached_kept) + "\n";
    return out;
}

std::string target_reach_report(const std::vector<std::string> &names, const std::vector<std::string> &genomes,
                                const std::vector<msspe_reach_record> &recs, uint32_t reach, int max_mismatches,
                                int exact_3p, bool scored, int mode, float tm_threshold)
{
    uint64_t columns = 0, plus = 0, minus = 0, either = 0, both = 0, gapped = 0;
    std::vector<uint64_t> starts(recs.size());
    for (size_t r = 0; r < recs.size(); ++r) {
        starts[r] = r ? starts[r - 1] + genomes[r - 1].size() + 1 : 0;
        columns += genomes[r].size();
        plus += recs[r].reached_plus;
        minus += recs[r].reached_minus;
        either += recs[r].reached_either;
        both += recs[r].reached_both;
        gapped += recs[r].gap_either_len > reach;
    }
    std::string out = "\nTarget reach (extension " + std::to_string(reach) + " bases; sites: " +
                      reach_rule(max_mismatches, exact_3p, scored, mode, tm_threshold) + "):\n";
    out += "  Total: " + std::to_string(recs.size()) + " genomes, " + std::to_string(columns) + " columns, reached plus " +
           std::to_string(plus) + ", minus " + std::to_string(minus) + ", either " + std::to_string(either) + ", both " +
           std::to_string(both) + "\n";
    out += "  Genomes with a gap above " + std::to_string(reach) + ": " + std::to_string(gapped) + "\n";
    std::vector<size_t> order(recs.size());
    for (size_t r = 0; r < order.size(); ++r) order[r] = r;
    std::stable_sort(order.begin(), order.end(),
                     [&](size_t a, size_t b) { return recs[a].gap_either_len > recs[b].gap_either_len; });
    order.resize(std::min<size_t>(20, order.size()));
    out += "  Longest gaps, " + std::to_string(order.size()) + " genomes (name: offset, length):\n";
    for (const size_t r : order)
        out += "    " + names[r] + ": " + std::to_string(recs[r].gap_either_pos - starts[r]) + ", " +
               std::to_string(recs[r].gap_either_len) + "\n";
    return out;
}

std::string target_reach_csv(const std::vector<std::string> &names, const std::vector<std::string> &genomes,
                             const std::vector<msspe_reach_record> &recs)
{
    std::string out = "name,columns,sites_plus,sites_minus,reached_plus,reached_minus,reached_either,reached_both,"
                      "gap_plus_len,gap_plus_pos,gap_minus_len,gap_minus_pos,gap_either_len,gap_either_pos\n";
    uint64_t start = 0;
    for (size_t r = 0; r < recs.size(); ++r) {
        const msspe_reach_record &c = recs[r];
        out += names[r] + "," + std::to_string(genomes[r].size());
        for (const uint64_t v : {(uint64_t)c.sites_plus, (uint64_t)c.sites_minus, (uint64_t)c.reached_plus,
                                 (uint64_t)c.reached_minus, (uint64_t)c.reached_either, (uint64_t)c.reached_both,
                                 (uint64_t)c.gap_plus_len, c.gap_plus_pos - start, (uint64_t)c.gap_minus_len,
                                 c.gap_minus_pos - start, (uint64_t)c.gap_either_len, c.gap_either_pos - start})
            out += "," + std::to_string(v);
        out += "\n";
        start += genomes[r].size() + 1;
    }
    return out;
}

std::string background_report_scored(const std::vector<std::string> &names,
                                     const std::vector<std::pair<uint64_t, uint64_t>> &sites,
                                     const std::vector<std::pair<uint64_t, uint64_t>> &stable, int max_mismatches,
                                     int exact_3p, int mode, float tm_threshold, int flank)
{
    char thr[64];
    std::snprintf(thr, sizeof thr, "%.2f", (double)tm_threshold);
    std::string out = "\nBackground sites (up to " + std::to_string(max_mismatches) + " mismatches, last " +
                      std::to_string(exact_3p) + " bases exact; stable: thal " + (mode == 2 ? "END1" : "ANY") +
                      " t >= " + thr + " C" + (flank > 0 ? ", template flank " + std::to_string(flank) : std::string()) +
                      "):\n";
    uint64_t plus = 0, minus = 0, s_plus = 0, s_minus = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        out += "  " + names[i] + ": plus " + std::to_string(sites[i].first) + ", minus " +
               std::to_string(sites[i].second) + ", stable plus " + std::to_string(stable[i].first) + ", minus " +
               std::to_string(stable[i].second) + "\n";
        plus += sites[i].first;
        minus += sites[i].second;
        s_plus += stable[i].first;
        s_minus += stable[i].second;
    }
    out += "  Total: " + std::to_string(names.size()) + " primers, plus " + std::to_string(plus) + ", minus " +
           std::to_string(minus) + ", stable plus " + std::to_string(s_plus) + ", minus " + std::to_string(s_minus) +
           "\n";
    return out;
}

std::string background_report(const std::vector<std::string> &names,
                              const std::vector<std::pair<uint64_t, uint64_t>> &sites, int max_mismatches,
                              int exact_3p)
{
    std::string out = "\nBackground sites (up to " + std::to_string(max_mismatches) + " mismatches, last " +
                      std::to_string(exact_3p) + " bases exact):\n";
    uint64_t plus = 0, minus = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        out += "  " + names[i] + ": plus " + std::to_string(sites[i].first) + ", minus " +
               std::to_string(sites[i].second) + "\n";
        plus += sites[i].first;
        minus += sites[i].second;
    }
    out += "  Total: " + std::to_string(names.size()) + " primers, plus " + std::to_string(plus) + ", minus " +
           std::to_string(minus) + "\n";
    return out;
}

std::string primers_csv(const std::vector<KmerStat> &fwd, const std::vector<KmerStat> &rev, size_t first_f,
                        size_t first_r, const std::map<std::string, int> *tubes)
{
    std::string out = tubes ? "direction,name,primers,gc,avg,std,tm,tube\n" : "direction,name,primers,gc,avg,std,tm\n";
    for (const auto *list : {&fwd, &rev}) {
        size_t idx = list == &fwd ? first_f : first_r;
        for (const auto &p : *list) {
            const char *d = p.direction == SEQ_DIR_FWD ? "F" : "R";
            out += std::string(d) + ",Primer_" + std::to_string(idx++) + "_" + d + "," + p.word + "," +
                   fmt("%.2f", (double)(p.gc_percent / 100.0f)) + "," + fmt("%.2f", (double)p.mean) + "," +
                   fmt("%.2f", (double)p.std) + "," + fmt("%.2f", (double)p.tm);
            if (tubes) {   // 1-based: a label for people
                const auto it = tubes->find(p.word);
                out += it != tubes->end() && it->second >= 0 ? "," + std::to_string(it->second + 1) : ",";
            }
            out += "\n";
        }
    }
    return out;
}

// ---------------------------------------------------------------------------------------------
// main.rs:596-861
// ---------------------------------------------------------------------------------------------
namespace {
// MSSPE_HOST_TIMING=1: wall time of the pipeline phases on stderr (development aid)
struct PhaseTimer {
    bool on = std::getenv("MSSPE_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[od-msspe-hip] %-28s %8.1f ms\n", what,
                     std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
    ~PhaseTimer() { lap("teardown"); }   // declared first in run(): destroyed after everything else
};
}  // namespace

// main.rs:127-146 align_sequences(): `mafft --auto --quiet --thread -1 --op 1.53 --ep 0.123 --jtt 200 <file>`
// as a child process, its stdout is the aligned FASTA.  Like the reference (Command::output()) the exit
// status is not looked at and stderr is discarded; a mafft that cannot be started panics with
// std::process's message.  Runs before the engine is created: no process that holds a GPU spawns anything.
std::string align_sequences(const std::string &filepath)
{
    int fds[2];
    if (::pipe(fds) != 0) throw Panic("failed to execute MAFFT: cannot create a pipe");
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_adddup2(&fa, fds[1], STDOUT_FILENO);
    posix_spawn_file_actions_addopen(&fa, STDERR_FILENO, "/dev/null", O_WRONLY, 0);
    posix_spawn_file_actions_addopen(&fa, STDIN_FILENO, "/dev/null", O_RDONLY, 0);
    posix_spawn_file_actions_addclose(&fa, fds[0]);
    posix_spawn_file_actions_addclose(&fa, fds[1]);
    const char *argv[] = {"mafft", "--auto", "--quiet", "--thread", "-1", "--op", "1.53", "--ep", "0.123",
                          "--jtt", "200", filepath.c_str(), nullptr};
    pid_t pid = 0;
    const int rc = ::posix_spawnp(&pid, "mafft", &fa, nullptr, const_cast<char *const *>(argv), environ);
    posix_spawn_file_actions_destroy(&fa);
    ::close(fds[1]);
    if (rc != 0) {
        ::close(fds[0]);
        throw Panic(std::string("failed to execute MAFFT: Os { code: ") + std::to_string(rc) + ", kind: " +
                    (rc == ENOENT ? "NotFound" : "Other") + ", message: \"" + std::strerror(rc) + "\" }");
    }
    std::string out;
    char buf[1 << 16];
    for (;;) {
        const ssize_t got = ::read(fds[0], buf, sizeof buf);
        if (got > 0) out.append(buf, (size_t)got);
        else if (got == 0 || errno != EINTR) break;
    }
    ::close(fds[0]);
    int status = 0;
    while (::waitpid(pid, &status, 0) < 0 && errno == EINTR) {
    }
    return out;
}

namespace {
// the records of a FASTA file: regular files are mapped and parsed in place (no copy of a multi-hundred-MB input);
// anything else (pipes) is read through a stream
std::vector<SequenceRecord> read_records(const std::string &path)
{
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("cannot read " + path);
    struct stat st;
    void *map = MAP_FAILED;
    if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0)
        map = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map != MAP_FAILED) {
        (void)::madvise(map, (size_t)st.st_size, MADV_SEQUENTIAL);
        auto records = to_records(static_cast<const char *>(map), (size_t)st.st_size);
        (void)::munmap(map, (size_t)st.st_size);
        ::close(fd);
        return records;
    }
    ::close(fd);
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + path);
    std::ostringstream all;
    all << f.rdbuf();
    return to_records(all.str());
}
}  // namespace

namespace {
// A candidate one of the filters dropped (--rejected-out; what a re-pick round bans)
struct Rejected {
    std::string word;
    uint8_t direction;
    int round;
    const char *reason;   // stage_b, background, panel_dimer, cover, select_conflict, select_unneeded
};
// What one pass from stage A to the cover keeps and drops
struct Selection {
    std::vector<KmerStat> good_f, good_r;
    std::vector<Rejected> rejected;
    std::map<std::string, int> tubes;   // --tubes
    std::string select_text;            // --select-by-coverage: the round's block
    std::string seeding_text;           // --seed-mismatches / --seed-tm: the block of a round that seeded
};

// Stage A (started from the state in which the panel's words are picked already, never picking an excluded word),
// stage B and its filter, the background drop, the screen against the panel and the cover (or the tubes): the
// primers that survive, and every candidate dropped on the way with the step that dropped it.  The panel is never
// dropped.  --keep-all true drops nothing.
Selection select_primers(Engine &eng, const DeviceAlignment &aln, const Args &args, const ProgramConfig &cfg,
                         const NtthalOptions &opts, std::unique_ptr<DeviceBackground> &background,
                         const std::vector<std::string> &panel_f, const std::vector<std::string> &panel_r,
                         const std::vector<std::string> &excl_f, const std::vector<std::string> &excl_r, int round,
                         PhaseTimer &timer, const std::vector<uint32_t> *genome_weights, const PrimerCostFn *costs)
{
    Selection sel;
    auto reject = [&](const KmerStat &s, const char *reason) {
        sel.rejected.push_back({s.word, s.direction, round, reason});
    };
    // --seed-mismatches / --seed-tm: a round with a panel seeds on what the panel covers under the rule
    const msspe_chem seed_chem = ntthal_chem(opts);   // (the chemistry --coverage-tm scores with)
    const int seed_mode = !args.seed_scored ? 0 : args.seed_thal == "end1" ? 2 : 1;
    const msspe_seed_rule rule = {args.seed_mismatches, args.seed_3p_exact, seed_mode, seed_mode ? &seed_chem : nullptr,
                                  args.seed_tm};
    const bool tolerant = args.seed_tolerant && (!panel_f.empty() || !panel_r.empty());
    size_t seed_covered[2] = {0, 0};
    const auto cand_both = find_candidates_kmers_both(eng, aln, cfg, args.window_size, args.overlap_size,
                                                      args.search_windows_size, panel_f, panel_r, excl_f, excl_r,
                                                      tolerant ? &rule : nullptr, seed_covered);
    if (tolerant) {
        const size_t L = aln.length();
        const size_t P = L < (size_t)args.window_size ? 0 : (L - (size_t)args.window_size) / (size_t)args.overlap_size + 1;
        sel.seeding_text = seed_report(args.seed_mismatches, args.seed_3p_exact, seed_mode, args.seed_tm, seed_covered[0],
                                       panel_f.size(), seed_covered[1], panel_r.size(), P * (size_t)aln.rows());
    }
    const auto &cand_f = cand_both.first, &cand_r = cand_both.second;
    timer.lap("stage A (both directions)");
    const auto stats_f = get_kmer_stats(eng, cand_f, cfg);
    const auto stats_r = get_kmer_stats(eng, cand_r, cfg);
    auto prim_f = cfg.keep_all ? stats_f : filter_kmers(stats_f, cfg);
    auto prim_r = cfg.keep_all ? stats_r : filter_kmers(stats_r, cfg);
    if (!cfg.keep_all)
        for (const auto &lists : {std::make_pair(&stats_f, &prim_f), std::make_pair(&stats_r, &prim_r)}) {
            std::set<std::string> passed;
            for (const auto &s : *lists.second) passed.insert(s.word);
            for (const auto &s : *lists.first)
                if (!passed.count(s.word)) reject(s, "stage_b");
        }

    timer.lap("stage B + filter");
    // --background: uploaded once; candidates with too many off-target sites go before the cross-dimer screen, so the
    // vertex cover never spends a removal on them (the panel is reported below but never dropped)
    const int bg_mode = args.background_thal == "end1" ? 2 : 1;
    if (!args.background.empty()) {
        if (!background) {
            const auto bg_records = read_records(args.background);
            if (bg_records.empty()) throw Panic("No sequences found in the background file");
            background.reset(new DeviceBackground(eng, bg_records));
        }
        if (args.max_background_sites >= 0 && !cfg.keep_all)
            for (auto *list : {&prim_f, &prim_r}) {
                std::vector<std::string> words;
                for (const auto &s : *list) words.push_back(s.word);
                // with --background-tm the limit applies to the sites that would hold the primer
                std::vector<std::pair<uint64_t, uint64_t>> sites;
                if (args.background_scored)
                    (void)background->scored(words, args.background_mismatches, args.background_3p_exact,
                                             ntthal_chem(opts), bg_mode, args.background_tm, sites,
                                             args.background_flank);
                else
                    sites = background->sites(words, args.background_mismatches, args.background_3p_exact);
                size_t kept = 0;
                for (size_t i = 0; i < list->size(); ++i)
                    if (sites[i].first + sites[i].second <= (uint64_t)args.max_background_sites)
                        (*list)[kept++] = (*list)[i];
                    else
                        reject((*list)[i], "background");
                list->resize(kept);
            }
        timer.lap("background upload + screen");
    }
    const bool select = args.select_by_coverage == "true";   // (its forced panel bars the new primers it conflicts with)
    if (cfg.check_cross_dimers && !cfg.keep_all && !select && (!panel_f.empty() || !panel_r.empty())) {
        // a new primer that dimerises with the panel is dropped before the vertex cover (the panel stays whole)
        std::vector<std::string> cands, all_panel(panel_f);
        all_panel.insert(all_panel.end(), panel_r.begin(), panel_r.end());
        for (const auto *list : {&prim_f, &prim_r})
            for (const auto &s : *list) cands.push_back(s.word);
        const auto bad = panel_conflicts(eng, cands, all_panel, opts);
        for (auto *list : {&prim_f, &prim_r}) {
            for (const auto &s : *list)
                if (bad.count(s.word)) reject(s, "panel_dimer");
            list->erase(std::remove_if(list->begin(), list->end(), [&](const KmerStat &s) { return bad.count(s.word) != 0; }),
                        list->end());
        }
        timer.lap("panel cross-dimer screen");
    }
    if (select) {   // --select-by-coverage: one screen and one selection take the place of the cover or the tubes
        const msspe_chem chem = ntthal_chem(opts);
        const int mode = !args.thin_scored ? 0 : args.thin_thal == "end1" ? 2 : 1;
        sel.select_text = select_panel_on_device(
            eng, aln, prim_f, prim_r, panel_f, panel_r, args.window_size, args.overlap_size, args.search_windows_size,
            args.kmer_size, args.thin_mismatches, args.thin_3p_exact, args.thin_min_gain, chem, mode, args.thin_tm,
            std::max(1, args.tubes), args.tubes > 0, cfg.check_cross_dimers, !cfg.check_self_dimers, opts.dg,
            sel.good_f, sel.good_r, sel.tubes,
            [&](const KmerStat &s, bool barred) { reject(s, barred ? "select_conflict" : "select_unneeded"); }, &opts,
            args.select_depth, genome_weights, costs);
        timer.lap("stage C + selection by coverage");
        return sel;
    }
    std::vector<std::string> primers;
    for (const auto &s : prim_f) primers.push_back(s.word);
    for (const auto &s : prim_r) primers.push_back(s.word);
    std::set<std::string> deleted;
    if (args.tubes > 0) {   // --tubes: the primers that fit no tube are what is dropped
        sel.tubes = conflict_tubes_on_device(eng, primers, opts, cfg, args.tubes);
        for (const auto &kv : sel.tubes)
            if (kv.second < 0) deleted.insert(kv.first);
    } else {
        deleted = args.cover_on_device == "true" ? conflict_cover_on_device(eng, primers, opts, cfg)
                                                 : vertex_cover(primers, run_ntthal(eng, primers, opts, cfg));
    }
    for (const auto *list : {&prim_f, &prim_r})
        for (const auto &p : *list) {
            if (cfg.keep_all || !deleted.count(p.word))
                (list == &prim_f ? sel.good_f : sel.good_r).push_back(p);
            else
                reject(p, "cover");
        }

    timer.lap("stage C + vertex cover");
    return sel;
}
}  // namespace

int run(const Args &args, std::string &stdout_text)
{
    PhaseTimer timer;
    // --existing-primers: the panel this run extends (read first: a bad file is a usage error before any work)
    std::pair<std::vector<std::string>, std::vector<std::string>> panel;
    if (!args.existing_primers.empty()) panel = read_panel(args.existing_primers, args.kmer_size);
    const auto &panel_f = panel.first, &panel_r = panel.second;
    std::pair<std::vector<std::string>, std::vector<std::string>> banned;   // --exclude-primers
    if (!args.exclude_primers.empty()) banned = read_panel(args.exclude_primers, args.kmer_size, "--exclude-primers");
    std::vector<SequenceRecord> records;
    if (args.do_align == "true") {   // the reference's default (config.rs:131-138)
        const std::string aligned = align_sequences(args.input);
        records = to_records(aligned);
        timer.lap("mafft");
    } else {
        records = read_records(args.input);
    }
    if (records.empty()) throw Panic("No sequences found in the input file");
    std::vector<uint32_t> genome_weights;   // --genome-weights: a bad file is a usage error before the device is touched
    if (!args.genome_weights.empty()) {
        size_t L = 0;   // the alignment's length and its partitions, as DeviceAlignment and the calls count them
        for (const auto &r : records) L = std::max(L, r.sequence.size());
        const size_t P = L < (size_t)args.window_size ? 0 : (L - (size_t)args.window_size) / (size_t)args.overlap_size + 1;
        genome_weights = read_genome_weights(args.genome_weights, records, args.default_genome_weight, P);
    }
    std::map<std::string, uint32_t> listed_costs;   // --primer-costs: likewise
    if (args.primer_costs_on && !args.primer_costs.empty())
        listed_costs = read_primer_costs(args.primer_costs, args.kmer_size);
    timer.lap("read + to_records");

    const int auto_mm = (int)std::min<size_t>(10, std::max<size_t>(1, (records.size() + 49) / 50));
    ProgramConfig cfg;
    cfg.max_iterations = args.max_iterations;
    cfg.max_mismatch_segments = args.max_mismatch_segments >= 0 ? args.max_mismatch_segments : auto_mm;
    cfg.keep_all = args.keep_all == "true";
    cfg.check_cross_dimers = args.check_cross_dimers == "true";
    cfg.check_self_dimers = args.check_self_dimers == "true";
    cfg.check_hairpin = args.check_hairpin == "true";
    cfg.tm_stddev = args.tm_stddev;
    cfg.disable_tm_stddev = args.disable_tm_stddev == "true";
    cfg.disable_min_max_tm = args.disable_min_max_tm == "true";
    cfg.primer_config = {args.kmer_size, args.min_tm, args.max_tm, args.max_self_dimer_any_tm,
                         args.max_self_dimer_end_tm, args.max_hairpin_tm};
    cfg.stddev_population = args.stddev_population;

    std::vector<int> devices;   // --devices 0,1,...: a group; otherwise the one context of --device
    for (size_t at = 0; at < args.devices.size();) {
        size_t comma = args.devices.find(',', at);
        if (comma == std::string::npos) comma = args.devices.size();
        const std::string tok = args.devices.substr(at, comma - at);
        char *end = nullptr;
        const long d = std::strtol(tok.c_str(), &end, 10);
        if (tok.empty() || *end || d < 0) throw UsageError("error: invalid value '" + args.devices + "' for '--devices'");
        devices.push_back((int)d);
        at = comma + 1;
    }
    if (!devices.empty() && args.cover_on_device == "true")
        throw UsageError("error: '--cover-on-device true' runs on one device and cannot be combined with '--devices'");
    std::unique_ptr<Engine> eng_owner(devices.empty() ? new Engine(args.device, args.params_path)
                                                      : new Engine(devices, args.params_path));
    Engine &eng = *eng_owner;
    const DeviceAlignment aln(eng, records);   // one upload for stage A (both directions) and the report
    timer.lap("engine + alignment upload");
    std::string kinds_text;   // --max-cross-dimer-end-tm: one line per screen of candidates under both rules
    const NtthalOptions opts{args.mv_conc, args.dv_conc, args.dntp_conc, args.dna_conc,
                             args.annealing_temp, args.delta_g_threshold, args.cross_dimer_end,
                             args.max_cross_dimer_end_tm, args.cross_dimer_end ? &kinds_text : nullptr};
    const int bg_mode = args.background_thal == "end1" ? 2 : 1;
    std::unique_ptr<DeviceBackground> background;   // --background: uploaded once, by the first round
    // Round 0 is the run itself: the user's panel and exclusions.  --repick-rounds: round r >= 1 keeps what passed
    // (the user's panel plus everything kept so far is its panel), bans what failed (the user's exclusions plus
    // everything rejected so far) and lets stage A fill the holes; kept primers are never removed by a later round.
    // --primer-costs / --background-site-cost: a primer's listed or default cost, plus the site cost times its
    // background sites, counted as --max-background-sites counts them (the first round has uploaded the background)
    const PrimerCostFn cost_fn = [&](const std::vector<std::string> &words) {
        std::vector<uint32_t> out(words.size());
        std::vector<std::pair<uint64_t, uint64_t>> sites(words.size(), {0, 0});
        if (args.background_site_cost && background) {
            if (args.background_scored)
                (void)background->scored(words, args.background_mismatches, args.background_3p_exact, ntthal_chem(opts),
                                         bg_mode, args.background_tm, sites, args.background_flank);
            else
                sites = background->sites(words, args.background_mismatches, args.background_3p_exact);
        }
        for (size_t i = 0; i < words.size(); ++i) {
            const auto it = listed_costs.find(words[i]);
            out[i] = primer_cost(it == listed_costs.end() ? args.default_primer_cost : it->second,
                                 args.background_site_cost, sites[i].first + sites[i].second);
        }
        return out;
    };
    const PrimerCostFn *costs = args.primer_costs_on ? &cost_fn : nullptr;
    std::vector<Selection> rounds;
    std::vector<std::string> kept_f(panel_f), kept_r(panel_r), ban_f(banned.first), ban_r(banned.second);
    std::string rounds_text;
    for (int round = 0;; ++round) {
        Selection s = select_primers(eng, aln, args, cfg, opts, background, kept_f, kept_r, ban_f, ban_r, round, timer,
                                     genome_weights.empty() ? nullptr : &genome_weights, costs);
        for (const auto &p : s.good_f) kept_f.push_back(p.word);
        for (const auto &p : s.good_r) kept_r.push_back(p.word);
        for (const auto &r : s.rejected) (r.direction == SEQ_DIR_FWD ? ban_f : ban_r).push_back(r.word);
        const size_t n_new = s.good_f.size() + s.good_r.size(), n_rej = s.rejected.size();
        rounds_text += s.seeding_text;
        rounds.push_back(std::move(s));
        if (args.repick_rounds > 0)
            rounds_text += "Re-pick round " + std::to_string(round) + ": " + std::to_string(n_new) + " new, " +
                           std::to_string(n_rej) + " rejected, " +
                           std::to_string(kept_f.size() + kept_r.size() - panel_f.size() - panel_r.size()) +
                           " kept so far\n";
        // a round that rejects nothing leaves no hole to fill; a re-pick round that finds no new primer ends the loop
        if (round >= args.repick_rounds || n_rej == 0 || (round > 0 && n_new == 0)) break;
    }
    std::vector<KmerStat> good_f, good_r;   // the final lists: round 0's primers, then each round's
    std::map<std::string, int> round_f, round_r;
    for (size_t r = 0; r < rounds.size(); ++r) {
        for (const auto &p : rounds[r].good_f) good_f.push_back(p), round_f[p.word] = (int)r;
        for (const auto &p : rounds[r].good_r) good_r.push_back(p), round_r[p.word] = (int)r;
    }
    const std::map<std::string, int> &tubes = rounds[0].tubes;   // (--tubes runs one round)
    if (!args.rejected_out.empty()) {
        std::ofstream rej(args.rejected_out, std::ios::binary);
        if (!rej) throw std::runtime_error("cannot write " + args.rejected_out);
        rej << "direction,name,primers,round,reason\n";
        size_t idx[2] = {0, 0};
        for (const auto &sel : rounds)
            for (const auto &r : sel.rejected) {
                const bool fwd = r.direction == SEQ_DIR_FWD;
                rej << (fwd ? "F" : "R") << ",Rejected_" << idx[fwd ? 0 : 1]++ << (fwd ? "_F," : "_R,") << r.word << ","
                    << r.round << "," << r.reason << "\n";
            }
    }

    std::string thin_text;   // --thin-panel: everything below sees the thinned lists
    if (args.thin_panel == "true") {
        const msspe_chem thin_chem = ntthal_chem(opts);   // --thin-tm: the chemistry --coverage-tm scores with
        thin_text = thin_panel_on_device(eng, aln, good_f, good_r, panel_f, panel_r, args.window_size, args.overlap_size,
                                         args.search_windows_size, args.kmer_size, args.thin_mismatches,
                                         args.thin_3p_exact, args.thin_min_gain, args.thin_scored ? &thin_chem : nullptr,
                                         args.thin_thal == "end1" ? 2 : 1, args.thin_tm, args.thin_depth,
                                         genome_weights.empty() ? nullptr : &genome_weights, costs);
        timer.lap("panel thinning");
    }
    // the report covers the panel and the new primers together; the CSV lists the new ones, numbered on from the panel
    std::vector<KmerStat> rep_f = good_f, rep_r = good_r;
    for (const auto &w : panel_f) rep_f.push_back(KmerStat{w, SEQ_DIR_FWD});
    for (const auto &w : panel_r) rep_r.push_back(KmerStat{w, SEQ_DIR_REV});
    stdout_text = rounds_text + coverage_report(eng, aln, rep_f, rep_r, records, args.window_size, args.overlap_size,
                                  args.search_windows_size, args.kmer_size);
    if (args.coverage_mismatches > 0)   // the same primers (panel included), matched within N mismatches
        stdout_text += coverage_report_mm(eng, aln, rep_f, rep_r, records, args.window_size, args.overlap_size,
                                          args.search_windows_size, args.kmer_size, args.coverage_mismatches,
                                          args.coverage_3p_exact);
    if (args.coverage_scored)   // the same primers again, every match within the prefilter scored with thal
        stdout_text += coverage_report_thal(eng, aln, rep_f, rep_r, records, args.window_size, args.overlap_size,
                                            args.search_windows_size, args.kmer_size, args.coverage_mismatches,
                                            args.coverage_3p_exact, ntthal_chem(opts),
                                            args.coverage_thal == "end1" ? 2 : 1, args.coverage_tm);
    stdout_text += thin_text;
    for (const auto &sel : rounds) stdout_text += sel.select_text;   // (with --tubes its block lists the tubes)
    stdout_text += kinds_text;
    if (args.tubes > 0 && args.select_by_coverage != "true") stdout_text += tubes_report(good_f, good_r, tubes, args.tubes);
    if (background) {   // the CSV's primers by their CSV names, the panel's by the numbers the CSV continues from
        std::vector<std::string> names, words;
        for (const auto *panel_list : {&panel_f, &panel_r}) {
            const bool fwd = panel_list == &panel_f;
            const auto &good = fwd ? good_f : good_r;
            for (size_t i = 0; i < panel_list->size() + good.size(); ++i) {
                names.push_back("Primer_" + std::to_string(i) + (fwd ? "_F" : "_R"));
                words.push_back(i < panel_list->size() ? (*panel_list)[i] : good[i - panel_list->size()].word);
            }
        }
        if (args.background_scored && args.background_amplicon_max >= 0) {   // one scored pass feeds both blocks
            std::vector<std::pair<uint64_t, uint64_t>> stable, amps;
            std::vector<msspe_amplicon> list;
            const auto sites = background->amplicons(words, args.background_mismatches, args.background_3p_exact,
                                                     ntthal_chem(opts), bg_mode, args.background_tm,
                                                     (uint32_t)args.background_amplicon_min,
                                                     (uint32_t)args.background_amplicon_max, stable, amps, list,
                                                     args.background_flank);
            stdout_text += background_report_scored(names, sites, stable, args.background_mismatches,
                                                    args.background_3p_exact, bg_mode, args.background_tm,
                                                    args.background_flank);
            stdout_text += background_report_amplicons(names, amps, list, *background,
                                                       (uint32_t)args.background_amplicon_min,
                                                       (uint32_t)args.background_amplicon_max);
        } else if (args.background_scored) {
            std::vector<std::pair<uint64_t, uint64_t>> stable;
            const auto sites = background->scored(words, args.background_mismatches, args.background_3p_exact,
                                                  ntthal_chem(opts), bg_mode, args.background_tm, stable,
                                                  args.background_flank);
            stdout_text += background_report_scored(names, sites, stable, args.background_mismatches,
                                                    args.background_3p_exact, bg_mode, args.background_tm,
                                                    args.background_flank);
        } else
            stdout_text += background_report(names, background->sites(words, args.background_mismatches,
                                                                      args.background_3p_exact),
                                             args.background_mismatches, args.background_3p_exact);
    }
    if (args.reach >= 0) {   // the run's own genomes against the primers the CSV gets, forward and reverse alike
        std::vector<std::string> words, names, genomes;
        for (const auto &p : good_f) words.push_back(p.word);
        for (const auto &p : good_r) words.push_back(p.word);
        for (const auto &r : records) names.push_back(r.name);
        const int reach_mode = args.reach_thal == "end1" ? 2 : 1;
        ReachThinning thinning;   // --thin-reach: the --existing-primers panel behind the CSV's primers, forced
        const bool thin_reach = args.thin_reach == "true";
        if (thin_reach) {
            thinning.min_gain = args.thin_reach_min_gain;
            thinning.forced.assign(words.size(), 0);
            for (const auto *panel_list : {&panel_f, &panel_r})
                for (const auto &w : *panel_list) words.push_back(w), thinning.forced.push_back(1);
        }
        const auto recs = target_reach(eng, records, words, args.kmer_size, args.reach_mismatches, args.reach_3p_exact,
                                       ntthal_chem(opts), reach_mode, args.reach_scored ? args.reach_tm : 0.0f,
                                       (uint32_t)args.reach, genomes, thin_reach ? &thinning : nullptr);
        if (thin_reach) {   // the dropped primers leave the lists the CSV is written from, as --thin-panel's do
            std::vector<KmerStat> kept_f, kept_r;
            for (size_t i = 0; i < good_f.size(); ++i)
                if (thinning.keep[i]) kept_f.push_back(good_f[i]);
            for (size_t i = 0; i < good_r.size(); ++i)
                if (thinning.keep[good_f.size() + i]) kept_r.push_back(good_r[i]);
            good_f.swap(kept_f);
            good_r.swap(kept_r);
            stdout_text += reach_thinning_report(thinning, (uint32_t)args.reach, args.reach_mismatches,
                                                 args.reach_3p_exact, args.reach_scored, reach_mode, args.reach_tm);
        }
        stdout_text += target_reach_report(names, genomes, recs, (uint32_t)args.reach, args.reach_mismatches,
                                           args.reach_3p_exact, args.reach_scored, reach_mode, args.reach_tm);
        if (!args.reach_out.empty()) {
            std::ofstream reach_file(args.reach_out, std::ios::binary);
            if (!reach_file) throw std::runtime_error("cannot write " + args.reach_out);
            reach_file << target_reach_csv(names, genomes, recs);
        }
        timer.lap("target reach");
    }
    std::ofstream out(args.output, std::ios::binary);
    if (!out) throw std::runtime_error("cannot write " + args.output);
    // round 0's rows, then each round's, numbered on (--thin-panel: the rows that are left of each)
    size_t first_f = panel_f.size(), first_r = panel_r.size();
    for (size_t r = 0; r < rounds.size(); ++r) {
        std::vector<KmerStat> rows_f, rows_r;
        for (const auto &p : good_f)
            if (round_f.at(p.word) == (int)r) rows_f.push_back(p);
        for (const auto &p : good_r)
            if (round_r.at(p.word) == (int)r) rows_r.push_back(p);
        const std::string csv = primers_csv(rows_f, rows_r, first_f, first_r, args.tubes > 0 ? &tubes : nullptr);
        out << (r == 0 ? csv : csv.substr(csv.find('\n') + 1));
        first_f += rows_f.size();
        first_r += rows_r.size();
    }
    timer.lap("coverage report + csv");
    return 0;
}

}  // namespace od_msspe
