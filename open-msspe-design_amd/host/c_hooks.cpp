// c_hooks.cpp -- extern "C" test hooks over the host layer (used by tests/ through ctypes).
#include <cstring>
#include <sstream>

#include "od_msspe.hpp"

using namespace od_msspe;

namespace {
int emit(const std::string &s, char *out, size_t cap)
{
    if (s.size() + 1 > cap) {   // -3: the caller's buffer is too small (and says so: it is left an empty string)
        if (cap) out[0] = '\0';
        return -3;
    }
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}
std::vector<std::string> lines(const char *text)
{
    std::vector<std::string> v;
    std::istringstream in(text ? text : "");
    std::string l;
    while (std::getline(in, l))
        if (!l.empty()) v.push_back(l);
    return v;
}
}  // namespace

extern "C" {

// returns 0 ok, 2 usage error, 101 panic, 1 other; message / report text in `out`
int odm_run_cli(int argc, const char *const *argv, char *out, size_t cap)
{
    try {
        const Args a = Args::parse(argc, argv);
        std::string report;
        const int rc = run(a, report);
        emit(report, out, cap);
        return rc;
    } catch (const UsageError &e) {
        emit(e.what(), out, cap);
        return 2;
    } catch (const Panic &e) {
        emit(e.what(), out, cap);
        return 101;
    } catch (const std::exception &e) {
        emit(e.what(), out, cap);
        return 1;
    }
}

// parse only: writes "key=value" lines of the resolved options
int odm_parse_args(int argc, const char *const *argv, char *out, size_t cap)
{
    try {
        const Args a = Args::parse(argc, argv);
        std::ostringstream o;
        o << "input=" << a.input << "\noutput=" << a.output << "\nkmer_size=" << a.kmer_size
          << "\nwindow_size=" << a.window_size << "\noverlap_size=" << a.overlap_size
          << "\nmax_mismatch_segments=" << a.max_mismatch_segments << "\nmax_iterations=" << a.max_iterations
          << "\nsearch_windows_size=" << a.search_windows_size << "\nmv_conc=" << a.mv_conc
          << "\ndelta_g_threshold=" << a.delta_g_threshold << "\nkeep_all=" << a.keep_all
          << "\ncheck_hairpin=" << a.check_hairpin << "\ndo_align=" << a.do_align
          << "\ntm_stddev=" << a.tm_stddev << "\ncover_on_device=" << a.cover_on_device << "\ntubes=" << a.tubes
          << "\ncoverage_mismatches=" << a.coverage_mismatches << "\ncoverage_3p_exact=" << a.coverage_3p_exact
          << "\nmax_cross_dimer_end_tm=" << a.max_cross_dimer_end_tm_text << "\ncoverage_tm=" << a.coverage_tm_text << "\ncoverage_thal=" << a.coverage_thal
          << "\nselect_by_coverage=" << a.select_by_coverage << "\nthin_panel=" << a.thin_panel << "\nthin_mismatches=" << a.thin_mismatches
          << "\nthin_3p_exact=" << a.thin_3p_exact << "\nthin_min_gain=" << a.thin_min_gain
          << "\nthin_depth=" << a.thin_depth << "\nselect_depth=" << a.select_depth
          << "\ngenome_weights=" << a.genome_weights << "\ndefault_genome_weight=" << a.default_genome_weight
          << "\nthin_tm=" << a.thin_tm_text << "\nthin_thal=" << a.thin_thal
          << "\nseed_mismatches=" << a.seed_mismatches << "\nseed_3p_exact=" << a.seed_3p_exact
          << "\nseed_tm=" << a.seed_tm_text << "\nseed_thal=" << a.seed_thal
          << "\nseed_tolerant=" << (a.seed_tolerant ? "true" : "false")
          << "\nbackground=" << a.background << "\nbackground_mismatches=" << a.background_mismatches
          << "\nbackground_3p_exact=" << a.background_3p_exact << "\nmax_background_sites=" << a.max_background_sites
          << "\nbackground_tm=" << a.background_tm_text << "\nbackground_thal=" << a.background_thal
          << "\nbackground_flank=" << a.background_flank
          << "\nprimer_costs=" << a.primer_costs << "\ndefault_primer_cost=" << a.default_primer_cost
          << "\nbackground_site_cost=" << a.background_site_cost
          << "\n";
        emit(o.str(), out, cap);
        return 0;
    } catch (const UsageError &e) {
        emit(e.what(), out, cap);
        return 2;
    }
}

// primers: one per line; edges: "a,b" per line (directed conflict a -> b).  Output: deleted
// primers, one per line, sorted.
int odm_vertex_cover(const char *primers_nl, const char *edges_nl, char *out, size_t cap)
{
    ConflictGraph g;
    const auto primers = lines(primers_nl);
    g.nodes = primers;
    for (const auto &e : lines(edges_nl)) {
        const size_t c = e.find(',');
        g.edges[e.substr(0, c)].insert(e.substr(c + 1));
    }
    std::string s;
    for (const auto &d : vertex_cover(primers, g)) s += d + "\n";
    return emit(s, out, cap);
}

// primers and edges as odm_vertex_cover.  Output: "word<TAB>tube" per primer in input order, tubes from 0, "-" for a
// primer in no tube (assign_tubes, the sequential rule of DESIGN.md 4.9).
int odm_assign_tubes(const char *primers_nl, const char *edges_nl, int max_tubes, char *out, size_t cap)
{
    ConflictGraph g;
    const auto primers = lines(primers_nl);
    g.nodes = primers;
    for (const auto &e : lines(edges_nl)) {
        const size_t c = e.find(',');
        g.edges[e.substr(0, c)].insert(e.substr(c + 1));
    }
    const auto tubes = assign_tubes(primers, g, max_tubes);
    std::string s;
    for (const auto &p : primers) {
        const int t = tubes.at(p);
        s += p + "\t" + (t < 0 ? std::string("-") : std::to_string(t)) + "\n";
    }
    return emit(s, out, cap);
}

// rows: n incidence rows of `words` 64-bit words each (bit s & 63 of word s >> 6: segment s); forced: n flags or
// NULL.  order / gains (n entries each) and keep (n) out; returns the number of picks (thin_panel, the sequential rule
// of DESIGN.md 4.10); covered_out[0] / [1]: segments covered by all rows / by the kept ones.
int odm_thin_panel(const uint64_t *rows, int n, int words, int min_gain, const uint8_t *forced, int *order, int *gains,
                   uint8_t *keep, long long *covered_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    const ThinResult t = thin_panel(r, min_gain, f);
    for (size_t i = 0; i < t.order.size(); ++i) {
        order[i] = t.order[i];
        gains[i] = t.gains[i];
    }
    for (int p = 0; p < n; ++p) keep[p] = (uint8_t)t.keep[(size_t)p];
    if (covered_out) {
        covered_out[0] = (long long)t.covered_all;
        covered_out[1] = (long long)t.covered_kept;
    }
    return (int)t.order.size();
}

// odm_thin_panel with weights[n_seg] (a uint32 per segment: bit s of a row) and min_gain in weight units; gains are
// weights (uint32).  sums_out[0..3]: segments covered by all rows / by the kept ones, then the weight of each
// (thin_panel_weighted, the sequential rule of DESIGN.md 4.17).
int odm_thin_panel_weighted(const uint64_t *rows, int n, int words, const uint32_t *weights, int n_seg,
                            long long min_gain, const uint8_t *forced, int *order, uint32_t *gains, uint8_t *keep,
                            unsigned long long *sums_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    WeightedSums sums;
    const ThinResult t = thin_panel_weighted(r, std::vector<uint32_t>(weights, weights + n_seg), min_gain, f, sums);
    for (size_t i = 0; i < t.order.size(); ++i) {
        order[i] = t.order[i];
        gains[i] = sums.gains[i];
    }
    for (int p = 0; p < n; ++p) keep[p] = (uint8_t)t.keep[(size_t)p];
    if (sums_out) {
        sums_out[0] = t.covered_all;
        sums_out[1] = t.covered_kept;
        sums_out[2] = sums.weight_all;
        sums_out[3] = sums.weight_kept;
    }
    return (int)t.order.size();
}

// odm_thin_panel's arguments plus n_seg (segments: bits of a row), depth and shadow (n flags or NULL: primers that
// repeat a word and count in nothing).  depth_all / depth_kept (n_seg bytes each, or NULL) and counts_out[0..4] out:
// segments with depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >= depth, and the rounds.  Returns the
// number of picks (thin_panel_depth, the sequential rule of DESIGN.md 4.15).
int odm_thin_panel_depth(const uint64_t *rows, int n, int words, int n_seg, int depth, int min_gain,
                         const uint8_t *forced, const uint8_t *shadow, int *order, int *gains, uint8_t *keep,
                         uint8_t *depth_all, uint8_t *depth_kept, long long *counts_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f, sh;
    if (forced) f.assign(forced, forced + n);
    if (shadow) sh.assign(shadow, shadow + n);
    const ThinDepthResult t = thin_panel_depth(r, (size_t)n_seg, depth, min_gain, f, sh);
    for (size_t i = 0; i < t.order.size(); ++i) {
        order[i] = t.order[i];
        gains[i] = t.gains[i];
    }
    for (int p = 0; p < n; ++p) keep[p] = (uint8_t)t.keep[(size_t)p];
    for (int s = 0; s < n_seg; ++s) {
        if (depth_all) depth_all[s] = t.depth_all[(size_t)s];
        if (depth_kept) depth_kept[s] = t.depth_kept[(size_t)s];
    }
    if (counts_out) {
        for (int i = 0; i < 4; ++i) counts_out[i] = t.counts[i];
        counts_out[4] = t.rounds;
    }
    return (int)t.order.size();
}

// primers: forward words then reverse words, one per line each; forced: flags over both or NULL.  shadow_out[n]
// (thin_shadows); returns how many are shadows.
int odm_thin_shadows(const char *fwd_nl, const char *rev_nl, const uint8_t *forced, uint8_t *shadow_out)
{
    const auto fwd = lines(fwd_nl), rev = lines(rev_nl);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + fwd.size() + rev.size());
    const auto sh = thin_shadows(fwd, rev, f);
    int count = 0;
    for (size_t p = 0; p < sh.size(); ++p) {
        shadow_out[p] = (uint8_t)sh[p];
        count += sh[p];
    }
    return count;
}

// rows, forced, order, gains, keep as odm_thin_panel.  bitmap: n rows of ceil(n / 64) words, bit u of row p = the
// directed conflict p -> u (padding bits ignored); with drop_self the diagonal is not read (the nodes are named by
// index, so nobody has a reverse-complement partner).  tube[n]: the tube of a pick, -1 otherwise; barred[n];
// counts_out[0..3]: segments covered by all rows / by the kept ones, tubes in use, rounds.  Returns the number of picks
// (select_panel, the sequential rule of DESIGN.md 4.13).
int odm_select_panel(const uint64_t *rows, int n, int words, const uint64_t *bitmap, int max_tubes, int min_gain,
                     const uint8_t *forced, int drop_self, int *order, int *gains, uint8_t *keep, int *tube,
                     uint8_t *barred, long long *counts_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    std::vector<std::string> names((size_t)n);
    for (int p = 0; p < n; ++p) names[(size_t)p] = std::to_string(p);
    ConflictGraph g;
    g.nodes = names;
    const int W = (n + 63) / 64;
    for (int p = 0; p < n; ++p)
        for (int u = 0; u < n; ++u)
            if ((bitmap[(size_t)p * W + (u >> 6)] >> (u & 63)) & 1ull)
                if (!(drop_self && p == u)) g.edges[names[(size_t)p]].insert(names[(size_t)u]);
    const SelectResult s = select_panel(r, names, g, max_tubes, min_gain, f);
    for (size_t i = 0; i < s.order.size(); ++i) {
        order[i] = s.order[i];
        gains[i] = s.gains[i];
    }
    for (int p = 0; p < n; ++p) {
        keep[p] = (uint8_t)s.keep[(size_t)p];
        tube[p] = s.tube[(size_t)p];
        barred[p] = (uint8_t)s.barred[(size_t)p];
    }
    if (counts_out) {
        counts_out[0] = (long long)s.covered_all;
        counts_out[1] = (long long)s.covered_kept;
        counts_out[2] = s.tubes_used;
        counts_out[3] = s.rounds;
    }
    return (int)s.order.size();
}

// odm_select_panel with weights[n_seg] and min_gain in weight units; gains are weights (uint32).  sums_out[0..5]:
// segments covered by all rows / by the kept ones, tubes in use, rounds, then the weight covered by all rows / by the
// kept ones (select_panel_weighted, the sequential rule of DESIGN.md 4.17).
int odm_select_panel_weighted(const uint64_t *rows, int n, int words, const uint64_t *bitmap, const uint32_t *weights,
                              int n_seg, int max_tubes, long long min_gain, const uint8_t *forced, int drop_self,
                              int *order, uint32_t *gains, uint8_t *keep, int *tube, uint8_t *barred,
                              unsigned long long *sums_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    std::vector<std::string> names((size_t)n);
    for (int p = 0; p < n; ++p) names[(size_t)p] = std::to_string(p);
    ConflictGraph g;
    g.nodes = names;
    const int W = (n + 63) / 64;
    for (int p = 0; p < n; ++p)
        for (int u = 0; u < n; ++u)
            if ((bitmap[(size_t)p * W + (u >> 6)] >> (u & 63)) & 1ull)
                if (!(drop_self && p == u)) g.edges[names[(size_t)p]].insert(names[(size_t)u]);
    WeightedSums sums;
    const SelectResult s = select_panel_weighted(r, names, g, std::vector<uint32_t>(weights, weights + n_seg),
                                                 max_tubes, min_gain, f, sums);
    for (size_t i = 0; i < s.order.size(); ++i) {
        order[i] = s.order[i];
        gains[i] = sums.gains[i];
    }
    for (int p = 0; p < n; ++p) {
        keep[p] = (uint8_t)s.keep[(size_t)p];
        tube[p] = s.tube[(size_t)p];
        barred[p] = (uint8_t)s.barred[(size_t)p];
    }
    if (sums_out) {
        sums_out[0] = s.covered_all;
        sums_out[1] = s.covered_kept;
        sums_out[2] = (unsigned long long)s.tubes_used;
        sums_out[3] = (unsigned long long)s.rounds;
        sums_out[4] = sums.weight_all;
        sums_out[5] = sums.weight_kept;
    }
    return (int)s.order.size();
}

// odm_thin_panel_weighted with costs[n] (a uint32 >= 1 per row); weights may be NULL (a gain is a count then).
// sums_out[0..5]: segments covered by all rows / by the kept ones, the weight of each (without weights: the counts
// again), the costs of all rows / of the kept ones (thin_panel_cost, the sequential rule of DESIGN.md 4.18).
int odm_thin_panel_cost(const uint64_t *rows, int n, int words, const uint32_t *weights, int n_seg,
                        const uint32_t *costs, long long min_gain, const uint8_t *forced, int *order, uint32_t *gains,
                        uint8_t *keep, unsigned long long *sums_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    std::vector<uint32_t> w;
    if (weights) w.assign(weights, weights + n_seg);
    CostSums sums;
    const ThinResult t = thin_panel_cost(r, weights ? &w : nullptr, std::vector<uint32_t>(costs, costs + n), min_gain, f,
                                         sums);
    for (size_t i = 0; i < t.order.size(); ++i) {
        order[i] = t.order[i];
        gains[i] = sums.gains[i];
    }
    for (int p = 0; p < n; ++p) keep[p] = (uint8_t)t.keep[(size_t)p];
    if (sums_out) {
        sums_out[0] = t.covered_all;
        sums_out[1] = t.covered_kept;
        sums_out[2] = sums.weight_all;
        sums_out[3] = sums.weight_kept;
        sums_out[4] = sums.cost_all;
        sums_out[5] = sums.cost_kept;
    }
    return (int)t.order.size();
}

// odm_select_panel_weighted with costs[n]; weights may be NULL.  sums_out[0..7]: odm_select_panel_weighted's six, then
// the costs of all rows / of the kept ones (select_panel_cost, the sequential rule of DESIGN.md 4.18).
int odm_select_panel_cost(const uint64_t *rows, int n, int words, const uint64_t *bitmap, const uint32_t *weights,
                          int n_seg, const uint32_t *costs, int max_tubes, long long min_gain, const uint8_t *forced,
                          int drop_self, int *order, uint32_t *gains, uint8_t *keep, int *tube, uint8_t *barred,
                          unsigned long long *sums_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    std::vector<std::string> names((size_t)n);
    for (int p = 0; p < n; ++p) names[(size_t)p] = std::to_string(p);
    ConflictGraph g;
    g.nodes = names;
    const int W = (n + 63) / 64;
    for (int p = 0; p < n; ++p)
        for (int u = 0; u < n; ++u)
            if ((bitmap[(size_t)p * W + (u >> 6)] >> (u & 63)) & 1ull)
                if (!(drop_self && p == u)) g.edges[names[(size_t)p]].insert(names[(size_t)u]);
    std::vector<uint32_t> w;
    if (weights) w.assign(weights, weights + n_seg);
    CostSums sums;
    const SelectResult s = select_panel_cost(r, names, g, weights ? &w : nullptr,
                                             std::vector<uint32_t>(costs, costs + n), max_tubes, min_gain, f, sums);
    for (size_t i = 0; i < s.order.size(); ++i) {
        order[i] = s.order[i];
        gains[i] = sums.gains[i];
    }
    for (int p = 0; p < n; ++p) {
        keep[p] = (uint8_t)s.keep[(size_t)p];
        tube[p] = s.tube[(size_t)p];
        barred[p] = (uint8_t)s.barred[(size_t)p];
    }
    if (sums_out) {
        sums_out[0] = s.covered_all;
        sums_out[1] = s.covered_kept;
        sums_out[2] = (unsigned long long)s.tubes_used;
        sums_out[3] = (unsigned long long)s.rounds;
        sums_out[4] = sums.weight_all;
        sums_out[5] = sums.weight_kept;
        sums_out[6] = sums.cost_all;
        sums_out[7] = sums.cost_kept;
    }
    return (int)s.order.size();
}

// odm_select_panel's arguments plus n_seg and depth.  layer[i]: the layer of pick i; depth_all / depth_kept (n_seg bytes
// each, or NULL); counts_out[0..6]: segments with depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >=
// depth, then tubes in use, rounds, layers.  Returns the number of picks (select_panel_depth).
int odm_select_panel_depth(const uint64_t *rows, int n, int words, int n_seg, const uint64_t *bitmap, int depth,
                           int max_tubes, int min_gain, const uint8_t *forced, int drop_self, int *order, int *gains,
                           int *layer, uint8_t *keep, int *tube, uint8_t *barred, uint8_t *depth_all,
                           uint8_t *depth_kept, long long *counts_out)
{
    std::vector<std::vector<uint64_t>> r((size_t)n);
    for (int p = 0; p < n; ++p) r[(size_t)p].assign(rows + (size_t)p * words, rows + (size_t)(p + 1) * words);
    std::vector<char> f;
    if (forced) f.assign(forced, forced + n);
    std::vector<std::string> names((size_t)n);
    for (int p = 0; p < n; ++p) names[(size_t)p] = std::to_string(p);
    ConflictGraph g;
    g.nodes = names;
    const int W = (n + 63) / 64;
    for (int p = 0; p < n; ++p)
        for (int u = 0; u < n; ++u)
            if ((bitmap[(size_t)p * W + (u >> 6)] >> (u & 63)) & 1ull)
                if (!(drop_self && p == u)) g.edges[names[(size_t)p]].insert(names[(size_t)u]);
    const SelectDepthResult s = select_panel_depth(r, names, g, (size_t)n_seg, depth, max_tubes, min_gain, f);
    for (size_t i = 0; i < s.order.size(); ++i) {
        order[i] = s.order[i];
        gains[i] = s.gains[i];
        layer[i] = s.layer[i];
    }
    for (int p = 0; p < n; ++p) {
        keep[p] = (uint8_t)s.keep[(size_t)p];
        tube[p] = s.tube[(size_t)p];
        barred[p] = (uint8_t)s.barred[(size_t)p];
    }
    for (int i = 0; i < n_seg; ++i) {
        if (depth_all) depth_all[i] = s.depth_all[(size_t)i];
        if (depth_kept) depth_kept[i] = s.depth_kept[(size_t)i];
    }
    if (counts_out) {
        for (int i = 0; i < 4; ++i) counts_out[i] = s.counts[i];
        counts_out[4] = s.tubes_used;
        counts_out[5] = s.rounds;
        counts_out[6] = s.layers;
    }
    return (int)s.order.size();
}

// The block od-msspe-hip --thin-panel true --thin-tm T prints (thin_thal_report), from figures the caller has.  Needs no
// device.
int odm_thin_thal_block(int mode, float tm_threshold, int max_mismatches, int exact_3p, int min_gain,
                        long long kept_f, long long n_f, long long kept_r, long long n_r, long long forced,
                        long long held_all, long long held_kept, long long segments, char *out, size_t cap)
{
    return emit(thin_thal_report(mode, tm_threshold, max_mismatches, exact_3p, min_gain, (size_t)kept_f, (size_t)n_f,
                                 (size_t)kept_r, (size_t)n_r, (size_t)forced, (size_t)held_all, (size_t)held_kept,
                                 (size_t)segments), out, cap);
}

// The block a seeding round of od-msspe-hip --seed-mismatches M prints (seed_report), from figures the caller has.
// Needs no device.
int odm_seed_block(int max_mismatches, int exact_3p, int mode, float tm_threshold, long long covered_f, long long panel_f,
                   long long covered_r, long long panel_r, long long segments, char *out, size_t cap)
{
    return emit(seed_report(max_mismatches, exact_3p, mode, tm_threshold, (size_t)covered_f, (size_t)panel_f,
                            (size_t)covered_r, (size_t)panel_r, (size_t)segments), out, cap);
}

int odm_is_run(const char *kmer) { return is_run(kmer) ? 1 : 0; }

// primers: one per line -> the text the reference would pipe into ntthal (delta_g.rs:61-81)
int odm_format_ntthal_input(const char *primers_nl, int check_cross_dimers, int check_self_dimers, char *out,
                            size_t cap)
{
    ProgramConfig cfg{};
    cfg.check_cross_dimers = check_cross_dimers != 0;
    cfg.check_self_dimers = check_self_dimers != 0;
    return emit(format_ntthal_input(lines(primers_nl), cfg), out, cap);
}

// FASTA text -> "name\tsequence" lines
int odm_to_records(const char *fasta, char *out, size_t cap)
{
    std::string s;
    for (const auto &r : to_records(fasta)) s += r.name + "\t" + r.sequence + "\n";
    return emit(s, out, cap);
}

// rows: "word,direction,gc,mean,std,tm" per line, forward rows first
int odm_primers_csv(const char *rows_nl, char *out, size_t cap)
{
    std::vector<KmerStat> f, r;
    for (const auto &l : lines(rows_nl)) {
        std::istringstream in(l);
        std::string w, d, gc, mean, sd, tm;
        std::getline(in, w, ','); std::getline(in, d, ','); std::getline(in, gc, ',');
        std::getline(in, mean, ','); std::getline(in, sd, ','); std::getline(in, tm, ',');
        KmerStat k{w, (uint8_t)std::stoi(d), std::stof(gc), std::stof(mean), std::stof(sd), std::stof(tm),
                   true, 0, 0, 0, false};
        (k.direction == SEQ_DIR_FWD ? f : r).push_back(k);
    }
    return emit(primers_csv(f, r), out, cap);
}

// records: "name\tsequence" lines; fwd / rev: selected primer words, one per line.  The per-segment
// search runs on the device (there is no CPU version of it in the product).
int odm_coverage_report(const char *records_nl, const char *fwd_nl, const char *rev_nl, int segment,
                        int stride, int window, int k, char *out, size_t cap)
{
    std::vector<SequenceRecord> recs;
    for (const auto &l : lines(records_nl)) {
        const size_t t = l.find('\t');
        recs.push_back({l.substr(0, t), l.substr(t + 1)});
    }
    std::vector<KmerStat> f, r;
    for (const auto &w : lines(fwd_nl)) f.push_back({w, SEQ_DIR_FWD, 0, 0, 0, 0, true, 0, 0, 0, false});
    for (const auto &w : lines(rev_nl)) r.push_back({w, SEQ_DIR_REV, 0, 0, 0, 0, true, 0, 0, 0, false});
    try {
        Engine eng(0, "");
        return emit(coverage_report(eng, f, r, recs, segment, stride, window, k), out, cap);
    } catch (const std::exception &e) {
        emit(e.what(), out, cap);
        return -2;   // no usable GPU: the text is the reason
    }
}

// The block od-msspe-hip --coverage-mismatches N --coverage-3p-exact E prints after the exact report (the text of
// odm_coverage_report): segments covered within max_mismatches, the last exact_3p bases exact (msspe_segment_coverage_mm)
int odm_coverage_report_mm(const char *records_nl, const char *fwd_nl, const char *rev_nl, int segment, int stride,
                           int window, int k, int max_mismatches, int exact_3p, char *out, size_t cap)
{
    std::vector<SequenceRecord> recs;
    for (const auto &l : lines(records_nl)) {
        const size_t t = l.find('\t');
        recs.push_back({l.substr(0, t), l.substr(t + 1)});
    }
    std::vector<KmerStat> f, r;
    for (const auto &w : lines(fwd_nl)) f.push_back({w, SEQ_DIR_FWD, 0, 0, 0, 0, true, 0, 0, 0, false});
    for (const auto &w : lines(rev_nl)) r.push_back({w, SEQ_DIR_REV, 0, 0, 0, 0, true, 0, 0, 0, false});
    try {
        Engine eng(0, "");
        return emit(coverage_report_mm(eng, f, r, recs, segment, stride, window, k, max_mismatches, exact_3p), out,
                    cap);
    } catch (const std::exception &e) {
        emit(e.what(), out, cap);
        return -2;   // no usable GPU (or an engine error): the text is the reason
    }
}

// The block od-msspe-hip --coverage-tm prints (coverage_thal_block), from results the caller has: records as
// "name\tsequence" lines, held[record * P + partition] and the per-primer held counts.  Needs no device.
int odm_coverage_thal_block(const char *records_nl, int segment, int stride, const uint8_t *held,
                            const uint32_t *primer_held, int n_primers, int max_mismatches, int exact_3p, int mode,
                            float tm_threshold, char *out, size_t cap)
{
    std::vector<SequenceRecord> recs;
    size_t L = 0;
    for (const auto &l : lines(records_nl)) {
        const size_t t = l.find('\t');
        recs.push_back({l.substr(0, t), l.substr(t + 1)});
        L = std::max(L, recs.back().sequence.size());
    }
    const size_t P = L < (size_t)segment ? 0 : (L - (size_t)segment) / (size_t)stride + 1;
    return emit(coverage_thal_block(recs, P, segment, stride, held, primer_held, (size_t)n_primers, max_mismatches,
                                    exact_3p, mode, tm_threshold), out, cap);
}

float odm_tm_stat(const float *tm, int n, int population, float *std_out)
{
    std::vector<PrimerInfo> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i].tm = tm[i];
    float mean, sd;
    get_tm_stat(v, population != 0, mean, sd);
    *std_out = sd;
    return mean;
}

}  // extern "C"
