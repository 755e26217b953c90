"""ctypes binding of include/msspe_hip.h.  Fails loudly when the HIP library is missing."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent          # open-msspe-design_amd/
STATUS = {0: "MSSPE_OK", 1: "MSSPE_ERR_ARG", 2: "MSSPE_ERR_K", 3: "MSSPE_ERR_TABLES",
          4: "MSSPE_ERR_DEVICE", 5: "MSSPE_ERR_CAPACITY", 6: "MSSPE_ERR_NOMEM"}

# every symbol include/msspe_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "msspe_chem_ntthal_defaults", "msspe_chem_primer3_defaults", "msspe_create", "msspe_destroy",
    "msspe_last_error", "msspe_version", "msspe_set_option", "msspe_get_info", "msspe_kmer_trace", "msspe_set_stream", "msspe_reset_stream",
    "msspe_synchronize",
    "msspe_pack_oligos", "msspe_unpack_oligo", "msspe_cross_dimer_dev", "msspe_cross_dimer",
    "msspe_cross_dimer_edges_dev", "msspe_cross_dimer_edges", "msspe_cross_dimer_bound_dev", "msspe_cross_dimer_bound_list_dev", "msspe_cross_dimer_bound_list_packed_dev", "msspe_cross_dimer_bound_packed_dev", "msspe_cross_dimer_bound_window_dev", "msspe_host_bound_tables", "msspe_host_bound_packed", "msspe_host_bound_window", "msspe_host_bound_mirror_ok",
    "msspe_cross_dimer_ab_dev", "msspe_cross_dimer_ab_edges_dev", "msspe_cross_dimer_ab", "msspe_cross_dimer_ab_edges",
    "msspe_cross_dimer_edges_mixed",
    "msspe_cross_dimer_end_dev", "msspe_cross_dimer_end", "msspe_cross_dimer_end_edges_dev", "msspe_cross_dimer_end_edges",
    "msspe_cross_dimer_end_ab_dev", "msspe_cross_dimer_end_ab", "msspe_t_cut",
    "msspe_conflict_graph_dev", "msspe_conflict_graph_ab_dev", "msspe_conflict_graph_edges_dev",
    "msspe_conflict_graph_ab_edges_dev", "msspe_conflict_graph", "msspe_conflict_graph_edges",
    "msspe_conflict_graph_ab_edges",
    "msspe_conflict_cover_dev", "msspe_conflict_cover", "msspe_conflict_cover_rule",
    "msspe_conflict_tubes_dev", "msspe_conflict_tubes", "msspe_conflict_tubes_rule",
    "msspe_last_overflow_pairs", "msspe_pair_stage_stats", "msspe_pair_stage_samples", "msspe_host_pair_tables", "msspe_host_table_routes", "msspe_host_screen_plan", "msspe_host_slab_split", "msspe_host_split_tables", "msspe_device_put_rows", "msspe_segment_coverage", "msspe_segment_coverage_dev",
    "msspe_device_put", "msspe_device_get", "msspe_device_free", "msspe_thal_detail_pairs", "msspe_profile_enable", "msspe_profile_read",
    "msspe_oligo_stats_dev", "msspe_oligo_stats",
    "msspe_kmer_candidates", "msspe_kmer_candidates_dev", "msspe_round_g_f32",
    "msspe_packed_row_words", "msspe_device_put_rows_packed", "msspe_kmer_candidates_packed_dev",
    "msspe_kmer_candidates_both_packed_dev",
    "msspe_kmer_candidates_seeded", "msspe_kmer_candidates_seeded_packed_dev",
    "msspe_kmer_candidates_both_seeded_packed_dev",
    "msspe_kmer_candidates_sets", "msspe_kmer_candidates_sets_packed_dev", "msspe_kmer_candidates_both_sets_packed_dev",
    "msspe_kmer_candidates_tolerant", "msspe_kmer_candidates_tolerant_packed_dev",
    "msspe_kmer_candidates_both_tolerant_packed_dev",
    "msspe_segment_coverage_packed_dev",
    "msspe_segment_coverage_mm", "msspe_segment_coverage_mm_dev", "msspe_segment_coverage_mm_packed_dev",
    "msspe_segment_coverage_thal", "msspe_segment_coverage_thal_dev", "msspe_segment_coverage_thal_packed_dev",
    "msspe_panel_thin", "msspe_panel_thin_dev", "msspe_panel_thin_packed_dev",
    "msspe_panel_thin_thal", "msspe_panel_thin_thal_dev", "msspe_panel_thin_thal_packed_dev",
    "msspe_panel_thin_depth", "msspe_panel_thin_depth_dev", "msspe_panel_thin_depth_packed_dev",
    "msspe_panel_thin_thal_depth", "msspe_panel_thin_thal_depth_dev", "msspe_panel_thin_thal_depth_packed_dev",
    "msspe_panel_select", "msspe_panel_select_bitmap", "msspe_panel_select_dev", "msspe_panel_select_packed_dev",
    "msspe_panel_select_rule",
    "msspe_panel_select_depth", "msspe_panel_select_depth_bitmap", "msspe_panel_select_depth_dev",
    "msspe_panel_select_depth_packed_dev", "msspe_panel_select_depth_rule",
    "msspe_panel_thin_weighted", "msspe_panel_thin_weighted_dev", "msspe_panel_thin_weighted_packed_dev",
    "msspe_panel_select_weighted_dev", "msspe_panel_select_weighted_packed_dev", "msspe_panel_select_weighted_rule",
    "msspe_panel_thin_cost", "msspe_panel_thin_cost_dev", "msspe_panel_thin_cost_packed_dev",
    "msspe_panel_select_cost_dev", "msspe_panel_select_cost_packed_dev", "msspe_panel_select_cost_rule",
    "msspe_device_put_stream_packed", "msspe_background_sites_packed_dev", "msspe_background_sites",
    "msspe_background_thal_packed_dev", "msspe_background_thal",
    "msspe_background_amplicons_packed_dev", "msspe_background_amplicons",
    "msspe_background_thal_flank_packed_dev", "msspe_background_thal_flank",
    "msspe_background_amplicons_flank_packed_dev", "msspe_background_amplicons_flank",
    "msspe_stream_reach_packed_dev", "msspe_stream_reach",
    "msspe_panel_thin_reach_packed_dev", "msspe_panel_thin_reach",
    "msspe_round_fixed_f32", "msspe_g_cut",
    "msspe_group_create", "msspe_group_destroy", "msspe_group_last_error", "msspe_group_size",
    "msspe_group_transport", "msspe_group_transport_reason", "msspe_group_rccl_available", "msspe_group_member", "msspe_group_set_option", "msspe_group_rows",
    "msspe_cross_dimer_group", "msspe_cross_dimer_edges_group", "msspe_oligo_stats_group",
]


class MsspeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class Chem(C.Structure):
    """msspe_chem: what od-msspe passes to ntthal (od-msspe/src/delta_g.rs:93-110)."""
    _fields_ = [("mv", C.c_double), ("dv", C.c_double), ("dntp", C.c_double),
                ("dna_conc", C.c_double), ("temp_c", C.c_double), ("max_loop", C.c_int)]

    @classmethod
    def ntthal(cls, mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0, max_loop=30):
        return cls(mv, dv, dntp, dna_conc, temp_c, max_loop)

    @classmethod
    def primer3(cls, mv=50.0, dv=1.5, dntp=0.6, dna_conc=50.0, temp_c=37.0, max_loop=30):
        return cls(mv, dv, dntp, dna_conc, temp_c, max_loop)


class ConflictRule(C.Structure):
    """msspe_conflict_rule: which of the two pair rules count (thal ANY decided on dG, thal END1 decided on t; the row
    is oligo 1 of END1) and their thresholds.  dg_threshold / end_tm_threshold None: that rule is off."""
    _fields_ = [("use_any", C.c_int), ("dg_threshold", C.c_float),
                ("use_end", C.c_int), ("end_tm_threshold", C.c_float)]

    @classmethod
    def of(cls, dg_threshold: float | None = -9000.0, end_tm_threshold: float | None = None):
        return cls(int(dg_threshold is not None), 0.0 if dg_threshold is None else dg_threshold,
                   int(end_tm_threshold is not None), 0.0 if end_tm_threshold is None else end_tm_threshold)


KIND_ANY, KIND_END = 1, 2
KIND_EDGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("kinds", np.uint32), ("reserved", np.uint32)])


class KmerOpt(C.Structure):
    """msspe_kmer_opt: od-msspe/src/constants.rs:1-5 defaults."""
    _fields_ = [("segment_size", C.c_int), ("overlap_size", C.c_int),
                ("search_window_size", C.c_int), ("kmer_size", C.c_int),
                ("max_iterations", C.c_int), ("max_mismatch_segments", C.c_int)]


# msspe_site: one off-target site of the list msspe_background_sites* makes
SITE_DTYPE = np.dtype([("primer", np.uint32), ("pos", np.uint32), ("mismatches", np.uint16), ("strand", np.uint16)])


# msspe_scored_site: one off-target site with its thal score (msspe_background_thal*); dg and t are raw
SCORED_SITE_DTYPE = np.dtype([("primer", np.uint32), ("pos", np.uint32), ("mismatches", np.uint16),
                              ("strand", np.uint16), ("stable", np.uint32), ("dg", np.float64), ("t", np.float64)])
THAL_MODES = {"any": 1, "end1": 2}

# msspe_scored_match: one match of a primer in a target segment with its thal score (msspe_segment_coverage_thal*)
SCORED_MATCH_DTYPE = np.dtype([("primer", np.uint32), ("segment", np.uint32), ("offset", np.uint32),
                               ("mismatches", np.uint16), ("stable", np.uint16), ("dg", np.float64),
                               ("t", np.float64)])
assert SCORED_MATCH_DTYPE.itemsize == 32

# msspe_thal_detail: the full thal record of one pair (msspe_thal_detail_pairs), what ntthal prints per input line
THAL_DETAIL_DTYPE = np.dtype([("dS", np.float64), ("dH", np.float64), ("dG", np.float64), ("t", np.float64),
                              ("no_structure", np.int32), ("n_pairs", np.int32),
                              ("ps1", np.uint8, (32,)), ("ps2", np.uint8, (32,))])
assert THAL_DETAIL_DTYPE.itemsize == 104

# msspe_amplicon: a plus-strand stable site of primer fwd at pos and a minus-strand one of primer rev, len columns on
AMPLICON_DTYPE = np.dtype([("fwd", np.uint32), ("rev", np.uint32), ("pos", np.uint32), ("len", np.uint32)])


class AmpliconOpt(C.Structure):
    """msspe_amplicon_opt: product lengths (both primers included) that count, k <= min_len <= max_len."""
    _fields_ = [("min_len", C.c_uint32), ("max_len", C.c_uint32)]


# msspe_reach_record: what the stable sites of one record reach (msspe_stream_reach*); positions are stream positions
REACH_RECORD_DTYPE = np.dtype([(f, np.uint32) for f in (
    "sites_plus", "sites_minus", "reached_plus", "reached_minus", "reached_either", "reached_both",
    "gap_plus_len", "gap_plus_pos", "gap_minus_len", "gap_minus_pos", "gap_either_len", "gap_either_pos")])
assert REACH_RECORD_DTYPE.itemsize == 48


class ReachOpt(C.Structure):
    """msspe_reach_opt: the length of the extension product, the primer included, k <= reach < 2^31."""
    _fields_ = [("reach", C.c_uint32)]


class MismatchOpt(C.Structure):
    """msspe_mismatch_opt: coverage within max_mismatches, the primer's last exact_3p bases exact."""
    _fields_ = [("max_mismatches", C.c_int), ("exact_3p", C.c_int)]


class ThinOpt(C.Structure):
    """msspe_thin_opt: a pick must cover at least min_gain segments nothing kept covers yet."""
    _fields_ = [("min_gain", C.c_int)]


class ThinDepthOpt(C.Structure):
    """msspe_thin_depth_opt: min_gain as ThinOpt; every segment keeps min(depth, primers it has) primers (1..255)."""
    _fields_ = [("min_gain", C.c_int), ("depth", C.c_int)]


class SelectOpt(C.Structure):
    """msspe_select_opt: min_gain as ThinOpt, at most max_tubes (1..64) tubes, drop_self_pairs as the cover's."""
    _fields_ = [("min_gain", C.c_int), ("max_tubes", C.c_int), ("drop_self_pairs", C.c_int)]


class SelectDepthOpt(C.Structure):
    """msspe_select_depth_opt: SelectOpt's fields, then depth (1..255): layer r adds primers for the segments that
    still have fewer than r."""
    _fields_ = [("min_gain", C.c_int), ("max_tubes", C.c_int), ("drop_self_pairs", C.c_int), ("depth", C.c_int)]


def lib_path() -> Path:
    return PKG_DIR / "libmsspe_hip.so"


_lib_override: Path | None = None


def use_library(path) -> None:
    """Development aid (A/B timing of two builds, tools/perf_probe.py MSSPE_PROBE_LIB): load another build of the library; call before the
    first Engine is created."""
    global _lib_override
    _lib_override = Path(path)


_lib = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    try:                      # PyTorch ships its own HIP runtime; when it is used in the same
        import torch          # process it must be loaded first so that a single runtime exists
    except Exception:         # (torch is plumbing here: device buffers, streams, torch.distributed)
        pass
    p = _lib_override or lib_path()
    if not p.exists():
        raise ImportError(f"{p} is missing: build it with open-msspe-design_amd/build.sh "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(str(p))
    vp, u64p = C.c_void_p, C.c_void_p
    L.msspe_version.restype = C.c_char_p
    L.msspe_last_error.restype = C.c_char_p
    L.msspe_last_error.argtypes = [vp]
    L.msspe_create.argtypes = [C.c_int, C.c_char_p, C.POINTER(vp)]
    L.msspe_destroy.argtypes = [vp]
    L.msspe_set_stream.argtypes = [vp, vp]
    L.msspe_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.msspe_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_longlong)]
    L.msspe_kmer_trace.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_group_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.msspe_group_destroy.argtypes = [vp]
    L.msspe_group_destroy.restype = None
    L.msspe_group_last_error.argtypes = [vp]
    L.msspe_group_last_error.restype = C.c_char_p
    L.msspe_group_size.argtypes = [vp]
    L.msspe_group_transport.argtypes = [vp]
    L.msspe_group_transport.restype = C.c_char_p
    L.msspe_group_transport_reason.argtypes = [vp]
    L.msspe_group_transport_reason.restype = C.c_char_p
    L.msspe_group_rccl_available.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.msspe_group_member.argtypes = [vp, C.c_int]
    L.msspe_group_member.restype = vp
    L.msspe_group_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.msspe_group_rows.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_cross_dimer_group.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float, vp, vp]
    L.msspe_cross_dimer_edges_group.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float, vp,
                                                C.c_uint64, C.POINTER(C.c_uint64)]
    L.msspe_oligo_stats_group.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem)] + [vp] * 5
    L.msspe_reset_stream.argtypes = [vp]
    L.msspe_synchronize.argtypes = [vp]
    L.msspe_pack_oligos.argtypes = [C.c_char_p, C.c_int, C.c_int, u64p]
    L.msspe_unpack_oligo.argtypes = [C.c_uint64, C.c_int, C.c_char_p]
    L.msspe_cross_dimer_dev.argtypes = [vp, u64p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float,
                                        C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.msspe_cross_dimer.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float,
                                    vp, vp, vp, vp]
    L.msspe_cross_dimer_edges.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float, vp,
                                          C.c_uint64, C.POINTER(C.c_uint64)]
    L.msspe_cross_dimer_edges_dev.argtypes = [vp, u64p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float,
                                              C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_uint64, vp]
    L.msspe_cross_dimer_bound_dev.argtypes = [vp, u64p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float,
                                              C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.msspe_cross_dimer_bound_list_dev.argtypes = L.msspe_cross_dimer_bound_dev.argtypes
    L.msspe_cross_dimer_bound_list_packed_dev.argtypes = L.msspe_cross_dimer_bound_dev.argtypes
    L.msspe_cross_dimer_bound_packed_dev.argtypes = L.msspe_cross_dimer_bound_dev.argtypes
    L.msspe_cross_dimer_bound_window_dev.argtypes = L.msspe_cross_dimer_bound_dev.argtypes
    L.msspe_host_bound_window.argtypes = [C.c_char_p, C.POINTER(Chem), C.c_float, C.POINTER(C.c_int32)]
    L.msspe_host_bound_packed.argtypes = [C.c_char_p, C.POINTER(Chem), C.c_float, vp, vp, C.POINTER(C.c_int32)]
    L.msspe_host_bound_tables.argtypes = [C.c_char_p, C.POINTER(Chem), C.c_float, vp, vp, C.POINTER(C.c_int32)]
    L.msspe_host_bound_mirror_ok.argtypes = [C.c_char_p, C.POINTER(Chem), C.c_float, C.POINTER(C.c_int32)]
    L.msspe_cross_dimer_ab_dev.argtypes = [vp, u64p, C.c_int, C.c_int, u64p, C.c_int, C.c_int, C.POINTER(Chem),
                                           C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.msspe_cross_dimer_ab_edges_dev.argtypes = [vp, u64p, C.c_int, C.c_int, u64p, C.c_int, C.c_int, C.POINTER(Chem),
                                                 C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_uint64, vp]
    L.msspe_cross_dimer_ab.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                       C.POINTER(Chem), C.c_float, vp, vp, vp, vp]
    L.msspe_cross_dimer_ab_edges.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                             C.POINTER(Chem), C.c_float, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.msspe_cross_dimer_edges_mixed.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(Chem), C.c_float, vp,
                                                C.c_uint64, C.POINTER(C.c_uint64)]
    L.msspe_cross_dimer_end_dev.argtypes = L.msspe_cross_dimer_dev.argtypes
    L.msspe_cross_dimer_end.argtypes = L.msspe_cross_dimer.argtypes
    L.msspe_cross_dimer_end_edges_dev.argtypes = L.msspe_cross_dimer_edges_dev.argtypes
    L.msspe_cross_dimer_end_edges.argtypes = L.msspe_cross_dimer_edges.argtypes
    L.msspe_cross_dimer_end_ab_dev.argtypes = L.msspe_cross_dimer_ab_dev.argtypes
    L.msspe_cross_dimer_end_ab.argtypes = L.msspe_cross_dimer_ab.argtypes
    L.msspe_conflict_cover_dev.argtypes = [vp, u64p, C.c_int, C.c_int, u64p, C.c_int, vp, C.POINTER(C.c_int)]
    L.msspe_conflict_cover.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float, C.c_int, vp,
                                       C.POINTER(C.c_int)]
    rulep = C.POINTER(ConflictRule)
    L.msspe_conflict_graph_dev.argtypes = [vp, u64p, C.c_int, C.c_int, C.POINTER(Chem), rulep,
                                           C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.msspe_conflict_graph_edges_dev.argtypes = L.msspe_conflict_graph_dev.argtypes + [vp, C.c_uint64, vp]
    L.msspe_conflict_graph_ab_dev.argtypes = [vp, u64p, C.c_int, C.c_int, u64p, C.c_int, C.c_int, C.POINTER(Chem), rulep,
                                              C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.msspe_conflict_graph_ab_edges_dev.argtypes = L.msspe_conflict_graph_ab_dev.argtypes + [vp, C.c_uint64, vp]
    L.msspe_conflict_graph.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), rulep, vp, vp, vp]
    L.msspe_conflict_graph_edges.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), rulep, vp, C.c_uint64,
                                             C.POINTER(C.c_uint64)]
    L.msspe_conflict_graph_ab_edges.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                                C.POINTER(Chem), rulep, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.msspe_conflict_cover_rule.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), rulep, C.c_int, vp,
                                            C.POINTER(C.c_int)]
    L.msspe_conflict_tubes_rule.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), rulep, C.c_int, C.c_int,
                                            vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.msspe_conflict_tubes_dev.argtypes = [vp, u64p, C.c_int, C.c_int, u64p, C.c_int, C.c_int, vp, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]
    L.msspe_conflict_tubes.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_float, C.c_int, C.c_int,
                                       vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.msspe_last_overflow_pairs.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.msspe_pair_stage_stats.argtypes = [vp, C.POINTER(C.c_uint64)]   # out[16]
    L.msspe_pair_stage_samples.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]
    L.msspe_profile_enable.argtypes = [vp, C.c_int]
    L.msspe_profile_read.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.msspe_oligo_stats_dev.argtypes = [vp, u64p, C.c_int, C.c_int, C.POINTER(Chem)] + [vp] * 5
    L.msspe_oligo_stats.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem)] + [vp] * 5
    L.msspe_kmer_candidates.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.c_int,
                                        vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_kmer_candidates_dev.argtypes = L.msspe_kmer_candidates.argtypes
    L.msspe_kmer_candidates_packed_dev.argtypes = L.msspe_kmer_candidates.argtypes
    L.msspe_kmer_candidates_both_packed_dev.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), vp, vp,
                                                        C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), C.c_int]
    L.msspe_kmer_candidates_seeded.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.c_int, vp, C.c_int,
                                               vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_kmer_candidates_seeded_packed_dev.argtypes = L.msspe_kmer_candidates_seeded.argtypes
    L.msspe_kmer_candidates_both_seeded_packed_dev.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt),
                                                               vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_int),
                                                               vp, vp, C.POINTER(C.c_int), C.c_int]
    L.msspe_kmer_candidates_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.c_int,
                                             C.POINTER(KmerSets), vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_kmer_candidates_sets_packed_dev.argtypes = L.msspe_kmer_candidates_sets.argtypes
    L.msspe_kmer_candidates_both_sets_packed_dev.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt),
                                                             C.POINTER(KmerSets), C.POINTER(KmerSets), vp, vp,
                                                             C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), C.c_int]
    L.msspe_kmer_candidates_tolerant.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.c_int,
                                                 C.POINTER(KmerSets), C.POINTER(SeedRule), vp, vp, C.c_int,
                                                 C.POINTER(C.c_int), vp, vp]
    L.msspe_kmer_candidates_tolerant_packed_dev.argtypes = L.msspe_kmer_candidates_tolerant.argtypes
    L.msspe_kmer_candidates_both_tolerant_packed_dev.argtypes = [
        vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.POINTER(KmerSets), C.POINTER(KmerSets), C.POINTER(SeedRule),
        vp, vp, C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), C.c_int, vp, vp, vp, vp]
    L.msspe_packed_row_words.restype = C.c_size_t
    L.msspe_packed_row_words.argtypes = [C.c_size_t]
    L.msspe_device_put_rows_packed.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_size_t,
                                               C.POINTER(vp)]
    L.msspe_segment_coverage.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), vp, C.c_int, vp, C.c_int,
                                         vp]
    L.msspe_segment_coverage_dev.argtypes = L.msspe_segment_coverage.argtypes
    L.msspe_segment_coverage_packed_dev.argtypes = L.msspe_segment_coverage.argtypes
    L.msspe_segment_coverage_mm.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.POINTER(MismatchOpt),
                                            vp, C.c_int, vp, C.c_int, vp, vp]
    L.msspe_segment_coverage_mm_dev.argtypes = L.msspe_segment_coverage_mm.argtypes
    L.msspe_segment_coverage_mm_packed_dev.argtypes = L.msspe_segment_coverage_mm.argtypes
    L.msspe_segment_coverage_thal.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt),
                                              C.POINTER(MismatchOpt), vp, C.c_int, vp, C.c_int, C.POINTER(Chem),
                                              C.c_int, C.c_float, vp, vp, vp, vp, vp, C.c_uint64,
                                              C.POINTER(C.c_uint64)]
    L.msspe_segment_coverage_thal_dev.argtypes = L.msspe_segment_coverage_thal.argtypes
    L.msspe_segment_coverage_thal_packed_dev.argtypes = L.msspe_segment_coverage_thal.argtypes
    L.msspe_panel_thin.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.POINTER(MismatchOpt),
                                   C.POINTER(ThinOpt), u64p, C.c_int, u64p, C.c_int, vp, vp, vp, vp,
                                   C.POINTER(C.c_int), vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.msspe_device_put.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_void_p)]
    L.msspe_panel_thin_dev.argtypes = L.msspe_panel_thin.argtypes
    L.msspe_panel_thin_packed_dev.argtypes = L.msspe_panel_thin.argtypes
    L.msspe_panel_thin_thal.argtypes = (L.msspe_panel_thin.argtypes[:7] + [C.POINTER(Chem), C.c_int, C.c_float] +
                                        L.msspe_panel_thin.argtypes[7:])
    L.msspe_panel_thin_thal_dev.argtypes = L.msspe_panel_thin_thal.argtypes
    L.msspe_panel_thin_thal_packed_dev.argtypes = L.msspe_panel_thin_thal.argtypes
    # the sibling's arguments with ThinDepthOpt, then depth_all, depth_kept, counts
    L.msspe_panel_thin_depth.argtypes = (L.msspe_panel_thin.argtypes[:6] + [C.POINTER(ThinDepthOpt)] +
                                         L.msspe_panel_thin.argtypes[7:16] + [vp, vp, C.POINTER(C.c_longlong)])
    L.msspe_panel_thin_depth_dev.argtypes = L.msspe_panel_thin_depth.argtypes
    L.msspe_panel_thin_depth_packed_dev.argtypes = L.msspe_panel_thin_depth.argtypes
    L.msspe_panel_thin_thal_depth.argtypes = (L.msspe_panel_thin_depth.argtypes[:7] +
                                              [C.POINTER(Chem), C.c_int, C.c_float] +
                                              L.msspe_panel_thin_depth.argtypes[7:])
    L.msspe_panel_thin_thal_depth_dev.argtypes = L.msspe_panel_thin_thal_depth.argtypes
    L.msspe_panel_thin_thal_depth_packed_dev.argtypes = L.msspe_panel_thin_thal_depth.argtypes
    # alignment, n_seq, seq_len, opt, rule, sel, fwd, n_fwd, rev, n_rev, forced | graph | keep, order, gain, n_picked,
    # tube, barred, covered, covered_all, covered_kept, n_tubes_used
    select_in = [vp, vp, C.c_int, C.c_size_t, C.POINTER(KmerOpt), C.POINTER(SeedRule), C.POINTER(SelectOpt), u64p,
                 C.c_int, u64p, C.c_int, vp]
    select_out = [vp, vp, vp, C.POINTER(C.c_int), vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                  C.POINTER(C.c_int)]
    L.msspe_panel_select_dev.argtypes = select_in + [vp] + select_out
    L.msspe_panel_select_packed_dev.argtypes = select_in + [vp] + select_out
    L.msspe_panel_select_bitmap.argtypes = select_in + [vp] + select_out
    L.msspe_panel_select.argtypes = select_in + [C.POINTER(Chem), C.c_float] + select_out
    L.msspe_panel_select_rule.argtypes = select_in + [C.POINTER(Chem), rulep] + select_out
    # the selection's inputs with SelectDepthOpt | graph | keep, order, gain, n_picked, tube, barred, n_tubes_used,
    # pick_layer, depth_all, depth_kept, counts
    depth_in = select_in[:6] + [C.POINTER(SelectDepthOpt)] + select_in[7:]
    depth_out = [vp, vp, vp, C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), vp, vp, vp, C.POINTER(C.c_longlong)]
    L.msspe_panel_select_depth_dev.argtypes = depth_in + [vp] + depth_out
    L.msspe_panel_select_depth_packed_dev.argtypes = depth_in + [vp] + depth_out
    L.msspe_panel_select_depth_bitmap.argtypes = depth_in + [vp] + depth_out
    L.msspe_panel_select_depth.argtypes = depth_in + [C.POINTER(Chem), C.c_float] + depth_out
    L.msspe_panel_select_depth_rule.argtypes = depth_in + [C.POINTER(Chem), rulep] + depth_out
    # the weighted forms: the sibling's arguments with the weights behind the inputs and the two weight sums last
    wsums = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.msspe_panel_thin_weighted.argtypes = (L.msspe_panel_thin.argtypes[:12] + [vp] +
                                            L.msspe_panel_thin.argtypes[12:] + wsums)
    L.msspe_panel_thin_weighted_dev.argtypes = L.msspe_panel_thin_weighted.argtypes
    L.msspe_panel_thin_weighted_packed_dev.argtypes = L.msspe_panel_thin_weighted.argtypes
    L.msspe_panel_select_weighted_dev.argtypes = select_in + [vp, vp] + select_out + wsums
    L.msspe_panel_select_weighted_packed_dev.argtypes = select_in + [vp, vp] + select_out + wsums
    L.msspe_panel_select_weighted_rule.argtypes = select_in + [C.POINTER(Chem), rulep, vp] + select_out + wsums
    # the cost forms: the weighted sibling's arguments with the costs behind the weights and the two cost sums last
    L.msspe_panel_thin_cost.argtypes = (L.msspe_panel_thin.argtypes[:12] + [vp, vp] +
                                        L.msspe_panel_thin.argtypes[12:] + wsums + wsums)
    L.msspe_panel_thin_cost_dev.argtypes = L.msspe_panel_thin_cost.argtypes
    L.msspe_panel_thin_cost_packed_dev.argtypes = L.msspe_panel_thin_cost.argtypes
    L.msspe_panel_select_cost_dev.argtypes = select_in + [vp, vp, vp] + select_out + wsums + wsums
    L.msspe_panel_select_cost_packed_dev.argtypes = select_in + [vp, vp, vp] + select_out + wsums + wsums
    L.msspe_panel_select_cost_rule.argtypes = select_in + [C.POINTER(Chem), rulep, vp, vp] + select_out + wsums + wsums
    L.msspe_device_put_stream_packed.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int,
                                                 C.POINTER(vp), C.POINTER(C.c_size_t), vp]
    L.msspe_background_sites_packed_dev.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int,
                                                    vp, vp, C.c_uint64, vp]
    L.msspe_background_sites.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                         C.POINTER(MismatchOpt), u64p, C.c_int, vp, vp, C.c_uint64,
                                         C.POINTER(C.c_uint64), vp]
    L.msspe_background_thal_packed_dev.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int,
                                                   C.POINTER(Chem), C.c_int, C.c_float, vp, vp, vp, C.c_uint64, vp]
    L.msspe_background_thal.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                        C.POINTER(MismatchOpt), u64p, C.c_int, C.POINTER(Chem), C.c_int, C.c_float,
                                        vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.msspe_background_amplicons_packed_dev.argtypes = [
        vp, vp, C.c_size_t, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int, C.POINTER(Chem), C.c_int, C.c_float,
        C.POINTER(AmpliconOpt), vp, C.c_int, vp, vp, vp, C.POINTER(C.c_uint64), vp, C.c_uint64, vp]
    L.msspe_background_amplicons.argtypes = [
        vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int,
        C.POINTER(Chem), C.c_int, C.c_float, C.POINTER(AmpliconOpt), vp, vp, vp, C.POINTER(C.c_uint64), vp,
        C.c_uint64, C.POINTER(C.c_uint64), vp]
    # the _flank siblings: one int (flank) behind tm_threshold
    for name in ("msspe_background_thal_packed_dev", "msspe_background_thal", "msspe_background_amplicons_packed_dev",
                 "msspe_background_amplicons"):
        at = getattr(L, name).argtypes
        cut = at.index(C.c_float) + 1
        getattr(L, name.replace("_background_thal", "_background_thal_flank")
                .replace("_background_amplicons", "_background_amplicons_flank")).argtypes = at[:cut] + [C.c_int] + at[cut:]
    L.msspe_stream_reach_packed_dev.argtypes = [
        vp, vp, C.c_size_t, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int, C.POINTER(Chem), C.c_int, C.c_float,
        C.c_int, C.POINTER(ReachOpt), vp, C.c_int, vp, vp, vp]
    L.msspe_stream_reach.argtypes = [
        vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int,
        C.POINTER(Chem), C.c_int, C.c_float, C.c_int, C.POINTER(ReachOpt), vp, vp, vp, vp]
    L.msspe_panel_thin_reach_packed_dev.argtypes = [
        vp, vp, C.c_size_t, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int, C.POINTER(Chem), C.c_int, C.c_float,
        C.c_int, C.POINTER(ReachOpt), C.POINTER(ThinOpt), vp, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int), vp,
        C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), vp, vp, vp]
    L.msspe_panel_thin_reach.argtypes = [
        vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(MismatchOpt), u64p, C.c_int,
        C.POINTER(Chem), C.c_int, C.c_float, C.c_int, C.POINTER(ReachOpt), C.POINTER(ThinOpt), vp, vp, vp, vp,
        C.POINTER(C.c_int), vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), vp, vp, vp, vp]
    L.msspe_device_get.argtypes = [vp, vp, C.c_size_t, vp]
    L.msspe_host_table_routes.argtypes = [C.c_char_p, C.POINTER(Chem), C.POINTER(C.c_int32)]
    L.msspe_host_screen_plan.argtypes = [C.c_int] * 5 + [C.c_int64, vp, C.c_int, C.POINTER(C.c_int)]
    L.msspe_host_slab_split.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int,
                                        C.POINTER(C.c_int)]
    L.msspe_thal_detail_pairs.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(Chem), C.c_int, vp]
    L.msspe_round_g_f32.restype = C.c_float
    L.msspe_round_g_f32.argtypes = [C.c_double]
    L.msspe_round_fixed_f32.restype = C.c_float
    L.msspe_round_fixed_f32.argtypes = [C.c_double, C.c_int]
    L.msspe_g_cut.restype = C.c_double
    L.msspe_g_cut.argtypes = [C.c_float]
    L.msspe_t_cut.restype = C.c_double
    L.msspe_t_cut.argtypes = [C.c_float]
    _lib = L
    return L


def _words(x) -> np.ndarray:
    """Primer strings (or an array of packed words) -> contiguous uint64 packed words."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x)
    return pack_oligos(list(x)) if len(x) else np.zeros(0, dtype=np.uint64)


def _words_k(x, k: int | None):
    """Primer strings of one length (k read off them), or packed words with k given -> (uint64 words, k)."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        if k is None:
            raise ValueError("packed primer words need k=")
        return np.ascontiguousarray(x), k
    x = list(x)
    if not x and k is None:
        raise ValueError("an empty primer list needs k=")
    return _words(x), (len(x[0]) if x else k)


def pack_oligos(oligos) -> np.ndarray:
    """list[str] or uint8 (n,k) ASCII -> uint64[n] (2 bits per base, base p at bits 2p..2p+1)."""
    if isinstance(oligos, np.ndarray):
        n, k = oligos.shape
        buf = np.ascontiguousarray(oligos, dtype=np.uint8).tobytes()
    else:
        n = len(oligos)
        k = len(oligos[0]) if n else 0
        if any(len(o) != k for o in oligos):
            raise MsspeError(1, "oligos must all have the same length")
        buf = "".join(oligos).encode()
    out = np.zeros(n, dtype=np.uint64)
    rc = load_library().msspe_pack_oligos(buf, n, k, out.ctypes.data)
    if rc:
        raise MsspeError(rc, "pool holds characters other than ACGT" if rc == 1 else "bad oligo length")
    return out


def unpack_oligo(word: int, k: int) -> str:
    buf = C.create_string_buffer(k + 1)
    load_library().msspe_unpack_oligo(C.c_uint64(int(word)), k, buf)
    return buf.value.decode()


def round_g_f32(x: float) -> float:
    return float(load_library().msspe_round_g_f32(x))


def round_fixed_f32(x: float, decimals: int) -> float:
    return float(load_library().msspe_round_fixed_f32(x, decimals))


def g_cut(threshold: float) -> float:
    return float(load_library().msspe_g_cut(C.c_float(threshold)))


def t_cut(tm_threshold: float) -> float:
    """The END screen's cut: the largest x with round_fixed_f32(x, 2) < tm_threshold (msspe_t_cut)."""
    return float(load_library().msspe_t_cut(C.c_float(tm_threshold)))


# PRIMER_MAX_SELF_END_TH, the SELF_END limit od-msspe applies to each primer: the END screen's default
END_TM_THRESHOLD = 47.0


TABLE_ROUTE_KEYS = ("pair_tables", "fast_ok", "int_ok", "row_ok", "split_ok", "split_max_k", "wave_max_k")


def host_table_routes(params_path: str | None = None, chem: Chem | None = None) -> dict:
    """Which kernels the tables at params_path open at this chemistry (no device needed): msspe_host_table_routes."""
    out = (C.c_int32 * 8)()
    chem = chem or Chem.ntthal()
    rc = load_library().msspe_host_table_routes(str(params_path).encode() if params_path else None, C.byref(chem), out)
    if rc:
        raise MsspeError(rc, f"msspe_host_table_routes({params_path})")
    return dict(zip(TABLE_ROUTE_KEYS, list(out)[:7]))


FIRST_STAGES = ("dense", "wave", "split", "fast", "int", "row", "bound", "bound_mirror")   # csrc/screen_plan.hpp FirstStage
SCREEN_PLAN_COLUMNS = ("row0", "row1", "col0", "col1", "pairs", "list_entries", "flush_before")


def host_screen_plan(first_stage: str, row0: int, row1: int, col0: int, ncols: int, list_cap: int) -> np.ndarray:
    """The first-stage launches of a pair screen over rows [row0, row1) x ncols columns from col0 under hand-over lists
    of list_cap entries, as the screens execute them (no device needed): msspe_host_screen_plan.  int64 (launches, 7),
    columns SCREEN_PLAN_COLUMNS."""
    n = C.c_int(64)
    while True:
        out = np.zeros((n.value, 7), dtype=np.int64)
        rc = load_library().msspe_host_screen_plan(FIRST_STAGES.index(first_stage), row0, row1, col0, ncols, list_cap,
                                                   out.ctypes.data, len(out), C.byref(n))
        if rc == 0:
            return out[:n.value]
        if rc != 5:     # MSSPE_ERR_CAPACITY: n holds the launch count
            raise MsspeError(rc, f"msspe_host_screen_plan({first_stage}, {row0}, {row1}, {col0}, {ncols}, {list_cap})")


def host_slab_split(o0: int, o1: int, p0: int, p1: int, count: int, cap: int) -> np.ndarray:
    """The parts a thal-scored site pass lists again for the slab [o0, o1) x primers [p0, p1) whose count matches overran
    a work list of cap (count > cap), in the order they are pushed (no device needed): msspe_host_slab_split.  int64
    (parts, 4), columns o0, o1, p0, p1; no rows: one outer element against one primer cannot be split."""
    n = C.c_int(64)
    while True:
        out = np.zeros((n.value, 4), dtype=np.int64)
        rc = load_library().msspe_host_slab_split(o0, o1, p0, p1, count, cap, out.ctypes.data, len(out), C.byref(n))
        if rc == 0:
            return out[:n.value]
        if rc != 5:     # MSSPE_ERR_CAPACITY: n holds the part count
            raise MsspeError(rc, f"msspe_host_slab_split({o0}, {o1}, {p0}, {p1}, {count}, {cap})")


def host_bound_tables(params_path: str | None = None, chem: Chem | None = None, threshold: float = -9000.0) -> dict:
    """The bound first stage's tables (no device needed): msspe_host_bound_tables.  g / T in the layout of
    host_pair_tables' int_g / int_T, in units of 1 / unit_inv cal/mol, rounded down; >= void: not available."""
    g = np.zeros(2604, dtype=np.int32)
    T = np.zeros(239 * 64, dtype=np.int32)
    info = (C.c_int32 * 8)()
    chem = chem or Chem.ntthal()
    rc = load_library().msspe_host_bound_tables(str(params_path).encode() if params_path else None, C.byref(chem),
                                                C.c_float(threshold), g.ctypes.data, T.ctypes.data, info)
    if rc:
        raise MsspeError(rc, f"msspe_host_bound_tables({params_path})")
    keys = ("usable", "init", "cut", "unit_inv", "margin", "reach", "void", "max_k")
    return {"g": g, "T": T, **dict(zip(keys, list(info)))}


def host_bound_window(params_path: str | None = None, chem: Chem | None = None, threshold: float = -9000.0) -> dict:
    """The windowed packed instance's constants (option pair_bound_window; no device needed): msspe_host_bound_window.
    F: rows a cell scans exactly; ifar / bfar: the smallest finite entry of host_bound_packed's T over l1 >= F with
    l2 >= 1 / l2 = 0, `void` where there is none."""
    info = (C.c_int32 * 8)()
    chem = chem or Chem.ntthal()
    rc = load_library().msspe_host_bound_window(str(params_path).encode() if params_path else None, C.byref(chem),
                                                C.c_float(threshold), info)
    if rc:
        raise MsspeError(rc, f"msspe_host_bound_window({params_path})")
    return dict(zip(("usable", "F", "ifar", "bfar", "void"), list(info)))


def host_bound_packed(params_path: str | None = None, chem: Chem | None = None, threshold: float = -9000.0) -> dict:
    """The packed bound instance's tables (option pair_bound_packed; no device needed): msspe_host_bound_packed.
    g / T: host_bound_tables' entries floored to units of 2**(shift - 6) cal/mol, void entries as they are; a cell
    value + bias is the slot word's field, [lo, hi] the proven range of the values.  usable = 0: all else 0."""
    g = np.zeros(2604, dtype=np.int32)
    T = np.zeros(239 * 64, dtype=np.int32)
    info = (C.c_int32 * 8)()
    chem = chem or Chem.ntthal()
    rc = load_library().msspe_host_bound_packed(str(params_path).encode() if params_path else None, C.byref(chem),
                                                C.c_float(threshold), g.ctypes.data, T.ctypes.data, info)
    if rc:
        raise MsspeError(rc, f"msspe_host_bound_packed({params_path})")
    keys = ("usable", "shift", "bias", "lo", "hi", "init", "cut", "field_max")
    return {"g": g, "T": T, **dict(zip(keys, list(info)))}


def host_bound_mirror_ok(params_path: str | None = None, chem: Chem | None = None, threshold: float = -9000.0) -> bool:
    """May the bound first stage fill each unordered pair of a square screen once under these tables (option
    pair_mirror; no device needed)?  msspe_host_bound_mirror_ok."""
    ok = C.c_int32(0)
    chem = chem or Chem.ntthal()
    rc = load_library().msspe_host_bound_mirror_ok(str(params_path).encode() if params_path else None, C.byref(chem),
                                                   C.c_float(threshold), C.byref(ok))
    if rc:
        raise MsspeError(rc, f"msspe_host_bound_mirror_ok({params_path})")
    return bool(ok.value)


def _seed_words(seed, k: int, what: str = "seed") -> np.ndarray | None:
    """A seed= (or exclude=) list (strings of length k, ACGT) -> packed uint64 words; None when none was given."""
    if seed is None:
        return None
    seed = list(seed)
    for s in seed:
        if not isinstance(s, str) or len(s) != k:
            raise ValueError(f"{what} word {s!r} is not a string of length {k} (the k-mer size)")
    if not seed:
        return np.zeros(0, dtype=np.uint64)
    try:
        return pack_oligos(seed)
    except MsspeError as e:
        raise ValueError(f"{what} words must be ACGT only: {e}") from None


class KmerSets(C.Structure):
    """msspe_kmer_sets: a direction's seed and exclusion lists (host packed words)."""
    _fields_ = [("seed", C.c_void_p), ("n_seed", C.c_int), ("exclude", C.c_void_p), ("n_exclude", C.c_int)]


def _kmer_sets(seed: np.ndarray | None, exclude: np.ndarray | None) -> KmerSets:
    """The struct over two packed lists (None: empty); the arrays must outlive the call that reads it."""
    return KmerSets(seed.ctypes.data if seed is not None and len(seed) else None, 0 if seed is None else len(seed),
                    exclude.ctypes.data if exclude is not None and len(exclude) else None,
                    0 if exclude is None else len(exclude))


class SeedRule(C.Structure):
    """msspe_seed_rule: what a seed covers in a tolerant seeded run -- its matches within max_mismatches with the last
    exact_3p bases exact (mode 0), or those of them that thal scores stable at tm_threshold (mode 1 ANY, 2 END1)."""
    _fields_ = [("max_mismatches", C.c_int), ("exact_3p", C.c_int), ("mode", C.c_int), ("chem", C.POINTER(Chem)),
                ("tm_threshold", C.c_float)]


def seed_rule(max_mismatches: int, exact_3p: int, mode=0, chem: Chem | None = None,
              tm_threshold: float = 0.0) -> SeedRule:
    """mode: 0 | "any" / 1 | "end1" / 2.  The Chem is kept alive by the returned struct."""
    m = mode if isinstance(mode, int) else THAL_MODES[mode]
    r = SeedRule(max_mismatches, exact_3p, m, C.pointer(chem) if chem is not None else None, tm_threshold)
    r._chem = chem
    return r


def _ascii(oligos):
    if isinstance(oligos, np.ndarray):
        n, k = oligos.shape
        return np.ascontiguousarray(oligos, dtype=np.uint8).tobytes(), n, k
    n = len(oligos)
    k = len(oligos[0]) if n else 0
    return "".join(oligos).encode(), n, k


class Engine:
    """One msspe_ctx bound to one device."""

    def __init__(self, device: int = 0, params_path: str | None = None):
        self.L = load_library()
        self.ptr = C.c_void_p()
        rc = self.L.msspe_create(device, params_path.encode() if params_path else None,
                                 C.byref(self.ptr))
        if rc:
            msg = self.L.msspe_last_error(self.ptr).decode() if self.ptr else "allocation failed"
            if self.ptr:
                self.L.msspe_destroy(self.ptr)
                self.ptr = C.c_void_p()
            raise MsspeError(rc, msg)
        self.device = device

    def close(self):
        if getattr(self, "ptr", None):
            self.L.msspe_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())

    def set_stream(self, hip_stream: int | None):
        """Run on the caller's HIP stream (raw handle; 0/None = HIP's default stream)."""
        self._check(self.L.msspe_set_stream(self.ptr, C.c_void_p(hip_stream or 0)))

    def set_option(self, key: str, value) -> None:
        """Engine option (include/msspe_hip.h msspe_set_option); the library never reads the environment."""
        self._check(self.L.msspe_set_option(self.ptr, key.encode(), str(value).encode()))

    def info(self, key: str) -> int:
        """Facts about the device and the kernels the context will run (include/msspe_hip.h msspe_get_info)."""
        v = C.c_longlong(0)
        self._check(self.L.msspe_get_info(self.ptr, key.encode(), C.byref(v)))
        return int(v.value)

    def kmer_trace(self) -> np.ndarray:
        """Per winner of the last kmer_candidates call: (iteration, how it was selected) -- msspe_kmer_trace."""
        n = C.c_int(0)
        self._check(self.L.msspe_kmer_trace(self.ptr, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._check(self.L.msspe_kmer_trace(self.ptr, out.ctypes.data, int(out.size), C.byref(n)))
        out = out[:n.value]
        return np.stack([out >> 8, out & 0xff], axis=1)

    def reset_stream(self):
        self._check(self.L.msspe_reset_stream(self.ptr))

    def synchronize(self):
        self._check(self.L.msspe_synchronize(self.ptr))

    # ---- stage C ---------------------------------------------------------------------------
    def cross_dimer(self, pool, chem: Chem | None = None, threshold: float = -9000.0,
                    want_dg=True, want_tm=False, want_bitmap=True):
        """Host-buffer call: returns dict(row_conflicts, bitmap, dg, tm) for the full n x n matrix."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        words = (n + 63) // 64
        rc_ = np.zeros(n, dtype=np.uint32)
        bm = np.zeros((n, words), dtype=np.uint64) if want_bitmap else None
        dg = np.empty((n, n)) if want_dg else None
        tm = np.empty((n, n)) if want_tm else None
        self._check(self.L.msspe_cross_dimer(
            self.ptr, buf, n, k, C.byref(chem), C.c_float(threshold), rc_.ctypes.data,
            bm.ctypes.data if want_bitmap else None, dg.ctypes.data if want_dg else None,
            tm.ctypes.data if want_tm else None))
        return {"row_conflicts": rc_, "bitmap": bm, "dg": dg, "tm": tm}

    def cross_dimer_edges(self, pool, chem: Chem | None = None, threshold: float = -9000.0, capacity: int = 1 << 20):
        """Edge list of the whole pool: (edges structured array [a, b, dg], count); raises MsspeError
        (MSSPE_ERR_CAPACITY, .count = edges needed) when the capacity is too small."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        edges = np.zeros(capacity, dtype=np.dtype([("a", np.uint32), ("b", np.uint32), ("dg", np.float32)]))
        count = C.c_uint64()
        rc = self.L.msspe_cross_dimer_edges(self.ptr, buf, n, k, C.byref(chem), C.c_float(threshold),
                                            edges.ctypes.data, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count = int(count.value)
            err.edges = edges
            raise err
        return edges[:count.value], int(count.value)

    def cross_dimer_edges_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                              rows: tuple[int, int], cols: tuple[int, int], d_edges: int, capacity: int,
                              d_count: int, d_row_conflicts: int = 0):
        """Device-pointer edge list of a block (16-byte records a:u32, b:u32, dg:f64; *d_count may exceed
        the capacity = truncated); asynchronous."""
        self._check(self.L.msspe_cross_dimer_edges_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_edges), capacity, C.c_void_p(d_count)))

    def cross_dimer_bound_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                              rows: tuple[int, int], cols: tuple[int, int], d_bound: int):
        """Diagnostic (tests, debugging): the bound first stage's value of every pair of the block, float64 cal/mol
        into the caller's plane (+inf: no chain; -inf: not bounded there); asynchronous.  msspe_cross_dimer_bound_dev."""
        self._check(self.L.msspe_cross_dimer_bound_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_bound)))

    def cross_dimer_bound_window_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                                     rows: tuple[int, int], cols: tuple[int, int], d_bound: int):
        """cross_dimer_bound_packed_dev's plane from the windowed instance (option pair_bound_window): multiples of the
        same unit, at most the packed instance's values.  msspe_cross_dimer_bound_window_dev."""
        self._check(self.L.msspe_cross_dimer_bound_window_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_bound)))

    def cross_dimer_bound_packed_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                                     rows: tuple[int, int], cols: tuple[int, int], d_bound: int):
        """cross_dimer_bound_dev's plane from the packed instance of the bound first stage (option pair_bound_packed):
        values are multiples of its unit (host_bound_packed's shift).  msspe_cross_dimer_bound_packed_dev."""
        self._check(self.L.msspe_cross_dimer_bound_packed_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_bound)))

    def cross_dimer_bound_list_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                                   rows: tuple[int, int], cols: tuple[int, int], d_bound: int):
        """cross_dimer_bound_dev's plane with the bound list stage behind the first stage: every pair it bounds carries
        its value; -inf only for two self-complementary oligos and more than 63 stored cells.
        msspe_cross_dimer_bound_list_dev."""
        self._check(self.L.msspe_cross_dimer_bound_list_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_bound)))

    def cross_dimer_bound_list_packed_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                                          rows: tuple[int, int], cols: tuple[int, int], d_bound: int):
        """cross_dimer_bound_list_dev's plane from the packed instances of both stages (options pair_bound_packed and
        pair_bound_list_packed): values are multiples of the packed unit.  msspe_cross_dimer_bound_list_packed_dev."""
        self._check(self.L.msspe_cross_dimer_bound_list_packed_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_bound)))

    def cross_dimer_dev(self, d_pool: int, n: int, k: int, chem: Chem, threshold: float,
                        rows: tuple[int, int], cols: tuple[int, int], d_row_conflicts: int = 0,
                        d_bitmap: int = 0, d_dg: int = 0, d_tm: int = 0):
        """Device-pointer call (raw addresses, e.g. torch.Tensor.data_ptr()); asynchronous."""
        self._check(self.L.msspe_cross_dimer_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(threshold),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts),
            C.c_void_p(d_bitmap), C.c_void_p(d_dg), C.c_void_p(d_tm)))

    # ---- stage C, one pool against another (oligo lengths may differ) -------------------------
    def cross_dimer_ab(self, a, b, chem: Chem | None = None, threshold: float = -9000.0,
                       want_dg=True, want_tm=False, want_bitmap=True):
        """Ordered pairs (A[i], B[j]) of two pools, each of one length (msspe_cross_dimer_ab): the dict of
        cross_dimer with rows = A and columns = B (row_conflicts[n_a], bitmap (n_a, ceil(n_b/64)), dg / tm (n_a, n_b))."""
        abuf, n_a, k_a = _ascii(a)
        bbuf, n_b, k_b = _ascii(b)
        k_a, k_b = k_a or k_b or 2, k_b or k_a or 2   # an empty pool's length does not matter
        chem = chem or Chem.ntthal()
        rc_ = np.zeros(n_a, dtype=np.uint32)
        bm = np.zeros((n_a, (n_b + 63) // 64), dtype=np.uint64) if want_bitmap else None
        dg = np.empty((n_a, n_b)) if want_dg else None
        tm = np.empty((n_a, n_b)) if want_tm else None
        self._check(self.L.msspe_cross_dimer_ab(
            self.ptr, abuf, n_a, k_a, bbuf, n_b, k_b, C.byref(chem), C.c_float(threshold), rc_.ctypes.data,
            bm.ctypes.data if want_bitmap else None, dg.ctypes.data if want_dg else None,
            tm.ctypes.data if want_tm else None))
        return {"row_conflicts": rc_, "bitmap": bm, "dg": dg, "tm": tm}

    def cross_dimer_ab_dev(self, d_a: int, n_a: int, k_a: int, d_b: int, n_b: int, k_b: int, chem: Chem,
                           threshold: float, rows: tuple[int, int], cols: tuple[int, int], d_row_conflicts: int = 0,
                           d_bitmap: int = 0, d_dg: int = 0, d_tm: int = 0):
        """Device-pointer call over rows [rows) of A x columns [cols) of B (msspe_cross_dimer_ab_dev); asynchronous."""
        self._check(self.L.msspe_cross_dimer_ab_dev(
            self.ptr, C.c_void_p(d_a), n_a, k_a, C.c_void_p(d_b), n_b, k_b, C.byref(chem), C.c_float(threshold),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap),
            C.c_void_p(d_dg), C.c_void_p(d_tm)))

    def cross_dimer_ab_edges_dev(self, d_a: int, n_a: int, k_a: int, d_b: int, n_b: int, k_b: int, chem: Chem,
                                 threshold: float, rows: tuple[int, int], cols: tuple[int, int], d_edges: int,
                                 capacity: int, d_count: int, d_row_conflicts: int = 0):
        """Device-pointer edge list of a block of A x B (msspe_cross_dimer_ab_edges_dev: a = A index, b = B index);
        asynchronous."""
        self._check(self.L.msspe_cross_dimer_ab_edges_dev(
            self.ptr, C.c_void_p(d_a), n_a, k_a, C.c_void_p(d_b), n_b, k_b, C.byref(chem), C.c_float(threshold),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_edges), capacity,
            C.c_void_p(d_count)))

    def cross_dimer_ab_edges(self, a, b, chem: Chem | None = None, threshold: float = -9000.0,
                             capacity: int = 1 << 20):
        """Edge list of A x B (msspe_cross_dimer_ab_edges): (edges [a, b, dg] sorted by (a, b), dg as Edge::get_dg()
        reads it, count); raises MsspeError (MSSPE_ERR_CAPACITY, .count = edges needed) when the capacity is too
        small."""
        abuf, n_a, k_a = _ascii(a)
        bbuf, n_b, k_b = _ascii(b)
        k_a, k_b = k_a or k_b or 2, k_b or k_a or 2   # an empty pool's length does not matter
        chem = chem or Chem.ntthal()
        edges = np.zeros(capacity, dtype=np.dtype([("a", np.uint32), ("b", np.uint32), ("dg", np.float32)]))
        count = C.c_uint64()
        rc = self.L.msspe_cross_dimer_ab_edges(self.ptr, abuf, n_a, k_a, bbuf, n_b, k_b, C.byref(chem),
                                               C.c_float(threshold), edges.ctypes.data, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count = int(count.value)
            err.edges = edges
            raise err
        return edges[:count.value], int(count.value)

    def cross_dimer_edges_mixed(self, oligos, chem: Chem | None = None, threshold: float = -9000.0,
                                capacity: int = 1 << 20):
        """Edge list over every ordered pair of a pool whose oligos may differ in length (msspe_cross_dimer_edges_mixed):
        (edges [a, b, dg] sorted by (a, b), count), indices into `oligos`; capacity errors as cross_dimer_edges."""
        enc = [o.encode() for o in oligos]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        chem = chem or Chem.ntthal()
        edges = np.zeros(capacity, dtype=np.dtype([("a", np.uint32), ("b", np.uint32), ("dg", np.float32)]))
        count = C.c_uint64()
        rc = self.L.msspe_cross_dimer_edges_mixed(self.ptr, arr, len(enc), C.byref(chem), C.c_float(threshold),
                                                  edges.ctypes.data, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count = int(count.value)
            err.edges = edges
            raise err
        return edges[:count.value], int(count.value)

    # ---- the conflict graph under a pair of rules (thal ANY on dG, thal END1 on t; msspe_conflict_graph*) -----------
    def conflict_graph(self, pool, chem: Chem | None = None, rule: ConflictRule | None = None):
        """Whole pool under the rule (msspe_conflict_graph): dict(row_conflicts uint32[n], bitmap uint64 (n, ceil(n/64)),
        kind_counts uint64[3] = pairs that are ANY only, END only, both).  rule: ConflictRule.of(dg, end_tm)."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        rule = rule or ConflictRule.of()
        rc_ = np.zeros(n, dtype=np.uint32)
        bm = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
        kinds = np.zeros(3, dtype=np.uint64)
        self._check(self.L.msspe_conflict_graph(self.ptr, buf, n, k or 2, C.byref(chem), C.byref(rule), rc_.ctypes.data,
                                                bm.ctypes.data, kinds.ctypes.data))
        return {"row_conflicts": rc_, "bitmap": bm, "kind_counts": kinds}

    def conflict_graph_dev(self, d_pool: int, n: int, k: int, chem: Chem, rule: ConflictRule, rows: tuple[int, int],
                           cols: tuple[int, int], d_row_conflicts: int = 0, d_bitmap: int = 0, d_kind_counts: int = 0):
        """Device-pointer call over a block (msspe_conflict_graph_dev): row_conflicts uint32[n] +=, the bitmap block
        cleared and written, kind_counts uint64[3] +=; asynchronous."""
        self._check(self.L.msspe_conflict_graph_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.byref(rule), rows[0], rows[1], cols[0], cols[1],
            C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap), C.c_void_p(d_kind_counts)))

    def conflict_graph_ab_dev(self, d_a: int, n_a: int, k_a: int, d_b: int, n_b: int, k_b: int, chem: Chem,
                              rule: ConflictRule, rows: tuple[int, int], cols: tuple[int, int],
                              d_row_conflicts: int = 0, d_bitmap: int = 0, d_kind_counts: int = 0):
        """Rows [rows) of A (oligo 1 of the END rule) x columns [cols) of B (msspe_conflict_graph_ab_dev); asynchronous."""
        self._check(self.L.msspe_conflict_graph_ab_dev(
            self.ptr, C.c_void_p(d_a), n_a, k_a, C.c_void_p(d_b), n_b, k_b, C.byref(chem), C.byref(rule),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap),
            C.c_void_p(d_kind_counts)))

    def conflict_graph_edges_dev(self, d_pool: int, n: int, k: int, chem: Chem, rule: ConflictRule,
                                 rows: tuple[int, int], cols: tuple[int, int], d_edges: int, capacity: int,
                                 d_count: int, d_row_conflicts: int = 0, d_bitmap: int = 0, d_kind_counts: int = 0):
        """Device-pointer ordered edge list of a block (msspe_conflict_graph_edges_dev: 16-byte records a, b, kinds,
        reserved in ascending (a, b); *d_count may exceed the capacity = truncated); asynchronous."""
        self._check(self.L.msspe_conflict_graph_edges_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.byref(rule), rows[0], rows[1], cols[0], cols[1],
            C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap), C.c_void_p(d_kind_counts), C.c_void_p(d_edges), capacity,
            C.c_void_p(d_count)))

    def conflict_graph_ab_edges_dev(self, d_a: int, n_a: int, k_a: int, d_b: int, n_b: int, k_b: int, chem: Chem,
                                    rule: ConflictRule, rows: tuple[int, int], cols: tuple[int, int], d_edges: int,
                                    capacity: int, d_count: int, d_row_conflicts: int = 0, d_bitmap: int = 0,
                                    d_kind_counts: int = 0):
        """The A x B block as an ordered edge list (msspe_conflict_graph_ab_edges_dev: a = A index, b = B index)."""
        self._check(self.L.msspe_conflict_graph_ab_edges_dev(
            self.ptr, C.c_void_p(d_a), n_a, k_a, C.c_void_p(d_b), n_b, k_b, C.byref(chem), C.byref(rule),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap),
            C.c_void_p(d_kind_counts), C.c_void_p(d_edges), capacity, C.c_void_p(d_count)))

    def _kind_edges(self, call, capacity: int):
        edges = np.zeros(capacity, dtype=KIND_EDGE)
        count = C.c_uint64()
        rc = call(edges.ctypes.data if capacity else None, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count = int(count.value)
            err.edges = edges
            raise err
        return edges[:count.value], int(count.value)

    def conflict_graph_edges(self, pool, chem: Chem | None = None, rule: ConflictRule | None = None,
                             capacity: int = 1 << 20):
        """Ordered edge list of the whole pool under the rule (msspe_conflict_graph_edges): (edges [a, b, kinds,
        reserved] ascending in (a, b), count); raises MsspeError (MSSPE_ERR_CAPACITY, .count = edges needed, .edges =
        the first `capacity`) when the capacity is too small."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        rule = rule or ConflictRule.of()
        return self._kind_edges(lambda e, cap, cnt: self.L.msspe_conflict_graph_edges(
            self.ptr, buf, n, k or 2, C.byref(chem), C.byref(rule), e, cap, cnt), capacity)

    def conflict_graph_ab_edges(self, a, b, chem: Chem | None = None, rule: ConflictRule | None = None,
                                capacity: int = 1 << 20):
        """Ordered edge list of A x B under the rule (msspe_conflict_graph_ab_edges; A is oligo 1 of the END rule)."""
        abuf, n_a, k_a = _ascii(a)
        bbuf, n_b, k_b = _ascii(b)
        k_a, k_b = k_a or k_b or 2, k_b or k_a or 2   # an empty pool's length does not matter
        chem = chem or Chem.ntthal()
        rule = rule or ConflictRule.of()
        return self._kind_edges(lambda e, cap, cnt: self.L.msspe_conflict_graph_ab_edges(
            self.ptr, abuf, n_a, k_a, bbuf, n_b, k_b, C.byref(chem), C.byref(rule), e, cap, cnt), capacity)

    # ---- the greedy vertex cover of the conflict graph (od-msspe/src/main.rs:754-798; msspe_conflict_cover*) ------
    def conflict_cover(self, pool, chem: Chem | None = None, threshold: float = -9000.0,
                       drop_self_pairs: bool = False, end_tm_threshold: float | None = None) -> np.ndarray:
        """Screen a pool of distinct oligos of one length and cover its conflict graph on the device
        (msspe_conflict_cover): bool[n], True = removed by the reference's greedy cover.  drop_self_pairs: the
        reference's --check-self-dimers false.  Rounds of the call: info("cover_rounds").  end_tm_threshold: the graph is
        that of the rule (ANY at threshold, END at end_tm_threshold; msspe_conflict_cover_rule)."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        out = np.zeros(n, dtype=np.uint8)
        nd = C.c_int(0)
        if end_tm_threshold is not None:
            rule = ConflictRule.of(threshold, end_tm_threshold)
            self._check(self.L.msspe_conflict_cover_rule(self.ptr, buf, n, k or 2, C.byref(chem), C.byref(rule),
                                                         int(bool(drop_self_pairs)), out.ctypes.data, C.byref(nd)))
            return out.astype(bool)
        self._check(self.L.msspe_conflict_cover(self.ptr, buf, n, k or 2, C.byref(chem), C.c_float(threshold),
                                                int(bool(drop_self_pairs)), out.ctypes.data, C.byref(nd)))
        return out.astype(bool)

    def conflict_cover_dev(self, d_pool: int, n: int, k: int, d_bitmap: int, d_deleted: int,
                           drop_self_pairs: bool = False) -> int:
        """Device-pointer cover (msspe_conflict_cover_dev): d_bitmap n x ceil(n/64) uint64 as cross_dimer_dev writes
        the full block, d_deleted n bytes (1 = removed).  Returns the number of removed oligos; synchronises."""
        nd = C.c_int(0)
        self._check(self.L.msspe_conflict_cover_dev(self.ptr, C.c_void_p(d_pool), n, k, C.c_void_p(d_bitmap),
                                                    int(bool(drop_self_pairs)), C.c_void_p(d_deleted), C.byref(nd)))
        return int(nd.value)

    # ---- the conflict graph split into reaction tubes (engine extension; msspe_conflict_tubes*) --------------------
    def conflict_tubes(self, pool, chem: Chem | None = None, threshold: float = -9000.0, max_tubes: int = 8,
                       drop_self_pairs: bool = False, end_tm_threshold: float | None = None):
        """Screen a pool of distinct oligos of one length and split it into at most max_tubes (1..64) tubes in which
        no two oligos conflict (msspe_conflict_tubes): (uint8[n], tubes_used, unplaced); 255 (MSSPE_TUBE_NONE) marks an
        oligo in no tube.  Rounds of the call: info("tube_rounds").  end_tm_threshold: the graph is that of the rule (ANY at
        threshold, END at end_tm_threshold; msspe_conflict_tubes_rule)."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        out = np.zeros(n, dtype=np.uint8)
        used, unplaced = C.c_int(0), C.c_int(0)
        if end_tm_threshold is not None:
            rule = ConflictRule.of(threshold, end_tm_threshold)
            self._check(self.L.msspe_conflict_tubes_rule(self.ptr, buf, n, k or 2, C.byref(chem), C.byref(rule),
                                                         int(bool(drop_self_pairs)), int(max_tubes), out.ctypes.data,
                                                         C.byref(used), C.byref(unplaced)))
            return out, int(used.value), int(unplaced.value)
        self._check(self.L.msspe_conflict_tubes(self.ptr, buf, n, k or 2, C.byref(chem), C.c_float(threshold),
                                                int(bool(drop_self_pairs)), int(max_tubes), out.ctypes.data,
                                                C.byref(used), C.byref(unplaced)))
        return out, int(used.value), int(unplaced.value)

    def conflict_tubes_dev(self, d_pool: int, n: int, k: int, d_bitmap: int, d_tube: int, max_tubes: int,
                           drop_self_pairs: bool = False):
        """Device-pointer form (msspe_conflict_tubes_dev): d_bitmap as for conflict_cover_dev, d_tube n bytes.
        Returns (tubes_used, unplaced); synchronises."""
        used, unplaced = C.c_int(0), C.c_int(0)
        self._check(self.L.msspe_conflict_tubes_dev(self.ptr, C.c_void_p(d_pool), n, k, C.c_void_p(d_bitmap),
                                                    int(bool(drop_self_pairs)), int(max_tubes), C.c_void_p(d_tube),
                                                    C.byref(used), C.byref(unplaced)))
        return int(used.value), int(unplaced.value)

    # ---- stage C, 3'-end dimers (thal END1 for every ordered pair; include/msspe_hip.h msspe_cross_dimer_end*) ------
    def cross_dimer_end(self, pool, chem: Chem | None = None, tm_threshold: float = END_TM_THRESHOLD,
                        want_dg=True, want_tm=True, want_bitmap=True):
        """END screen of the whole pool (msspe_cross_dimer_end): dict(row_conflicts, bitmap, dg, tm); row i is oligo 1,
        the anchored 3' end.  A pair conflicts iff round_fixed_f32(max(0, t), 2) >= tm_threshold."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        rc_ = np.zeros(n, dtype=np.uint32)
        bm = np.zeros((n, (n + 63) // 64), dtype=np.uint64) if want_bitmap else None
        dg = np.empty((n, n)) if want_dg else None
        tm = np.empty((n, n)) if want_tm else None
        self._check(self.L.msspe_cross_dimer_end(
            self.ptr, buf, n, k, C.byref(chem), C.c_float(tm_threshold), rc_.ctypes.data,
            bm.ctypes.data if want_bitmap else None, dg.ctypes.data if want_dg else None,
            tm.ctypes.data if want_tm else None))
        return {"row_conflicts": rc_, "bitmap": bm, "dg": dg, "tm": tm}

    def cross_dimer_end_dev(self, d_pool: int, n: int, k: int, chem: Chem, tm_threshold: float,
                            rows: tuple[int, int], cols: tuple[int, int], d_row_conflicts: int = 0,
                            d_bitmap: int = 0, d_dg: int = 0, d_tm: int = 0):
        """Device-pointer END screen of a block (msspe_cross_dimer_end_dev); asynchronous."""
        self._check(self.L.msspe_cross_dimer_end_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(tm_threshold),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts),
            C.c_void_p(d_bitmap), C.c_void_p(d_dg), C.c_void_p(d_tm)))

    def cross_dimer_end_edges(self, pool, chem: Chem | None = None, tm_threshold: float = END_TM_THRESHOLD,
                              capacity: int = 1 << 20):
        """END edge list of the whole pool (msspe_cross_dimer_end_edges): (edges [a, b, t] sorted by (a, b), t =
        round_fixed_f32(max(0, t), 2), count); raises MsspeError (MSSPE_ERR_CAPACITY, .count = edges needed) when
        the capacity is too small."""
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        edges = np.zeros(capacity, dtype=np.dtype([("a", np.uint32), ("b", np.uint32), ("t", np.float32)]))
        count = C.c_uint64()
        rc = self.L.msspe_cross_dimer_end_edges(self.ptr, buf, n, k, C.byref(chem), C.c_float(tm_threshold),
                                                edges.ctypes.data, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count = int(count.value)
            err.edges = edges
            raise err
        return edges[:count.value], int(count.value)

    def cross_dimer_end_edges_dev(self, d_pool: int, n: int, k: int, chem: Chem, tm_threshold: float,
                                  rows: tuple[int, int], cols: tuple[int, int], d_edges: int, capacity: int,
                                  d_count: int, d_row_conflicts: int = 0):
        """Device-pointer END edge list of a block (16-byte records a:u32, b:u32, t:f64 raw; *d_count may exceed the
        capacity = truncated); asynchronous."""
        self._check(self.L.msspe_cross_dimer_end_edges_dev(
            self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem), C.c_float(tm_threshold), rows[0], rows[1], cols[0],
            cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_edges), capacity, C.c_void_p(d_count)))

    def cross_dimer_end_ab(self, a, b, chem: Chem | None = None, tm_threshold: float = END_TM_THRESHOLD,
                           want_dg=True, want_tm=True, want_bitmap=True):
        """END screen of the pairs (A[i], B[j]) (msspe_cross_dimer_end_ab): A is oligo 1, the anchored 3' end; the
        lengths may differ.  The dict of cross_dimer_end with rows = A and columns = B."""
        abuf, n_a, k_a = _ascii(a)
        bbuf, n_b, k_b = _ascii(b)
        k_a, k_b = k_a or k_b or 2, k_b or k_a or 2   # an empty pool's length does not matter
        chem = chem or Chem.ntthal()
        rc_ = np.zeros(n_a, dtype=np.uint32)
        bm = np.zeros((n_a, (n_b + 63) // 64), dtype=np.uint64) if want_bitmap else None
        dg = np.empty((n_a, n_b)) if want_dg else None
        tm = np.empty((n_a, n_b)) if want_tm else None
        self._check(self.L.msspe_cross_dimer_end_ab(
            self.ptr, abuf, n_a, k_a, bbuf, n_b, k_b, C.byref(chem), C.c_float(tm_threshold), rc_.ctypes.data,
            bm.ctypes.data if want_bitmap else None, dg.ctypes.data if want_dg else None,
            tm.ctypes.data if want_tm else None))
        return {"row_conflicts": rc_, "bitmap": bm, "dg": dg, "tm": tm}

    def cross_dimer_end_ab_dev(self, d_a: int, n_a: int, k_a: int, d_b: int, n_b: int, k_b: int, chem: Chem,
                               tm_threshold: float, rows: tuple[int, int], cols: tuple[int, int],
                               d_row_conflicts: int = 0, d_bitmap: int = 0, d_dg: int = 0, d_tm: int = 0):
        """Device-pointer END screen over rows [rows) of A x columns [cols) of B (msspe_cross_dimer_end_ab_dev);
        asynchronous."""
        self._check(self.L.msspe_cross_dimer_end_ab_dev(
            self.ptr, C.c_void_p(d_a), n_a, k_a, C.c_void_p(d_b), n_b, k_b, C.byref(chem), C.c_float(tm_threshold),
            rows[0], rows[1], cols[0], cols[1], C.c_void_p(d_row_conflicts), C.c_void_p(d_bitmap),
            C.c_void_p(d_dg), C.c_void_p(d_tm)))

    def pair_compl_end(self, pool, chem: Chem | None = None) -> np.ndarray:
        """n x n float64: max(t_end(a, b), t_end(b, a)), t_end = max(0, thal END1 t) -- both 3' ends of every pair
        (END2(a, b) = END1(b, a)), from one END screen and its transpose."""
        t = self.cross_dimer_end(pool, chem, want_dg=False, want_tm=True, want_bitmap=False)["tm"]
        t = np.maximum(t, 0.0)
        return np.maximum(t, t.T)

    def profile_enable(self, on: bool = True):
        self._check(self.L.msspe_profile_enable(self.ptr, int(on)))

    def profile_read(self) -> tuple[int, float]:
        """(launches of the all-pairs kernel, their summed device time in ms) since the last read."""
        n, ms = C.c_uint64(), C.c_double()
        self._check(self.L.msspe_profile_read(self.ptr, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def last_overflow_pairs(self) -> int:
        v = C.c_uint64()
        self._check(self.L.msspe_last_overflow_pairs(self.ptr, C.byref(v)))
        return int(v.value)

    def hand_over_lists(self) -> list[int]:
        """Pairs that entered each of the seven hand-over lists since the last read (msspe_get_info
        "hand_over_list_<q>"; include/msspe_hip.h names the stage that reads list q on each route); resets them."""
        return [self.info(f"hand_over_list_{q}") for q in range(7)]

    def segment_coverage(self, seqs: np.ndarray, opt: KmerOpt, fwd: list[str], rev: list[str]) -> np.ndarray:
        """uint8 (n_seq, P): 1 where the segment is covered by the primer set (main.rs:518-594)."""
        a = np.ascontiguousarray(seqs, dtype=np.uint8)
        n_seq, seq_len = a.shape
        P = 0 if seq_len < opt.segment_size else (seq_len - opt.segment_size) // opt.overlap_size + 1
        f = pack_oligos(fwd) if len(fwd) else np.zeros(0, dtype=np.uint64)
        r = pack_oligos(rev) if len(rev) else np.zeros(0, dtype=np.uint64)
        hit = np.zeros((n_seq, P), dtype=np.uint8)
        self._check(self.L.msspe_segment_coverage(
            self.ptr, a.ctypes.data, n_seq, seq_len, C.byref(opt), f.ctypes.data, len(f), r.ctypes.data, len(r),
            hit.ctypes.data))
        return hit

    def segment_coverage_mm(self, seqs: np.ndarray, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int,
                            per_primer: bool = False):
        """Coverage within max_mismatches, the primer's last exact_3p bases exact (msspe_segment_coverage_mm).
        seqs: uint8 (n_seq, L) host array; fwd / rev: primer strings (rev as the CSV writes it) or packed uint64 words.
        Returns best, uint8 (n_seq, P): the smallest mismatch count of a match in the segment, 255 when none; with
        per_primer, (best, counts): counts uint32 (len(fwd) + len(rev)) of segments each primer matches in."""
        a = np.ascontiguousarray(seqs, dtype=np.uint8)
        n_seq, seq_len = a.shape
        return self._coverage_mm(self.L.msspe_segment_coverage_mm, a.ctypes.data, n_seq, seq_len, opt, fwd, rev,
                                 max_mismatches, exact_3p, per_primer)

    def segment_coverage_mm_dev(self, d_seqs: int, n_seq: int, seq_len: int, opt: KmerOpt, fwd, rev,
                                max_mismatches: int, exact_3p: int, per_primer: bool = False):
        """As segment_coverage_mm on device bytes (n_seq x seq_len at address d_seqs)."""
        return self._coverage_mm(self.L.msspe_segment_coverage_mm_dev, C.c_void_p(d_seqs), n_seq, seq_len, opt, fwd,
                                 rev, max_mismatches, exact_3p, per_primer)

    def segment_coverage_mm_packed(self, d_packed: int, n_seq: int, seq_len: int, opt: KmerOpt, fwd, rev,
                                   max_mismatches: int, exact_3p: int, per_primer: bool = False):
        """As segment_coverage_mm on a packed alignment resident on the device (the handle put_rows_packed returns)."""
        return self._coverage_mm(self.L.msspe_segment_coverage_mm_packed_dev, C.c_void_p(d_packed), n_seq, seq_len,
                                 opt, fwd, rev, max_mismatches, exact_3p, per_primer)

    def _coverage_mm(self, fn, seqs_arg, n_seq, seq_len, opt, fwd, rev, max_mismatches, exact_3p, per_primer):
        P = 0 if seq_len < opt.segment_size else (seq_len - opt.segment_size) // opt.overlap_size + 1
        f, r = _words(fwd), _words(rev)
        best = np.zeros((n_seq, P), dtype=np.uint8)
        counts = np.zeros(len(f) + len(r), dtype=np.uint32)
        mm = MismatchOpt(max_mismatches, exact_3p)
        self._check(fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), C.byref(mm), f.ctypes.data, len(f),
                       r.ctypes.data, len(r), best.ctypes.data, counts.ctypes.data if per_primer else None))
        return (best, counts) if per_primer else best

    # ---- segment coverage scored with thal (engine extension; msspe_segment_coverage_thal*) -----------------------
    def segment_coverage_thal(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, chem: Chem,
                              mode, tm_threshold: float, *, matches: bool = False, capacity: int | None = None,
                              packed: str = "host"):
        """The matches of segment_coverage_mm, each scored with thal against the strand the primer anneals to
        (msspe_segment_coverage_thal*); mode "any" (1) or "end1" (2); a match is stable iff
        round_fixed_f32(max(0, t), 2) >= tm_threshold.  genomes: uint8 (n_seq, L) host array -- packed "host" hands
        it over as it is, "dev" and "packed" upload it first (as bytes / as packed rows) and call the device forms;
        or a resident alignment as (device address, n_seq, seq_len) with "dev" or "packed".  fwd / rev: primer strings
        (rev as the CSV writes it) or packed words.  Returns a dict: held uint8 (n_seq, P) (0 no match, 1 matches but
        none stable, 2 held), t_best float64 (n_seq, P), primer_segments and primer_held uint32 (forward primers
        first); with matches=True also "matches", a SCORED_MATCH_DTYPE array sorted by (primer, segment, offset),
        and "count".  capacity: the list's size (default: sized by a first call without a list); one below the
        number of matches raises MsspeError (MSSPE_ERR_CAPACITY) carrying .count, .result and the truncated
        .matches."""
        fn = {"host": self.L.msspe_segment_coverage_thal, "dev": self.L.msspe_segment_coverage_thal_dev,
              "packed": self.L.msspe_segment_coverage_thal_packed_dev}[packed]
        owned = None
        if isinstance(genomes, tuple):
            if packed == "host":
                raise ValueError("a resident alignment needs packed='dev' or 'packed'")
            handle, n_seq, seq_len = genomes
            seqs_arg = C.c_void_p(handle)
        else:
            a = np.ascontiguousarray(genomes, dtype=np.uint8)
            n_seq, seq_len = a.shape
            if packed == "host":
                seqs_arg = a.ctypes.data
            elif packed == "packed":
                owned = self.put_rows_packed(a)
                seqs_arg = C.c_void_p(owned)
            else:
                dev = C.c_void_p()
                self._check(self.L.msspe_device_put(self.ptr, a.ctypes.data, a.size, C.byref(dev)))
                owned = int(dev.value)
                seqs_arg = C.c_void_p(owned)
        try:
            P = 0 if seq_len < opt.segment_size else (seq_len - opt.segment_size) // opt.overlap_size + 1
            f, r = _words(fwd), _words(rev)
            n = len(f) + len(r)
            mm = MismatchOpt(max_mismatches, exact_3p)

            def call(recs, cap):
                out = {"held": np.zeros((n_seq, P), dtype=np.uint8), "t_best": np.zeros((n_seq, P), dtype=np.float64),
                       "primer_segments": np.zeros(n, dtype=np.uint32), "primer_held": np.zeros(n, dtype=np.uint32)}
                count = C.c_uint64(0)
                rc = fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), C.byref(mm), f.ctypes.data, len(f),
                        r.ctypes.data, len(r), C.byref(chem), self._thal_mode(mode), tm_threshold,
                        out["held"].ctypes.data, out["t_best"].ctypes.data, out["primer_segments"].ctypes.data,
                        out["primer_held"].ctypes.data, recs.ctypes.data if recs is not None else None, cap,
                        C.byref(count))
                return rc, out, int(count.value)

            if not matches:
                rc, out, _ = call(None, 0)
                self._check(rc)
                return out
            if capacity is None:   # the number of matches is the sum of no per-primer output: ask for it
                probe = np.zeros(1, dtype=SCORED_MATCH_DTYPE)
                rc, out, capacity = call(probe, 0)
                if rc not in (0, 5):
                    self._check(rc)
            recs = np.zeros(max(capacity, 1), dtype=SCORED_MATCH_DTYPE)
            rc, out, count = call(recs, capacity)
            if rc:
                err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
                err.count, err.result, err.matches = count, out, recs[:min(count, capacity)]
                raise err
            out["matches"], out["count"] = recs[:count], count
            return out
        finally:
            if owned is not None:
                self.device_free(owned)

    # ---- a panel thinned to the primers its coverage needs (engine extension; msspe_panel_thin*) -----------------
    def panel_thin(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, min_gain: int = 1,
                   forced=None, form: str = "host"):
        """Greedy set cover of the segments the primers match in within max_mismatches, the last exact_3p bases
        exact (msspe_panel_thin*).  genomes: uint8 (n_seq, L) host array -- form "host" hands it over as it is, "dev"
        and "packed" upload it first (as bytes / as packed rows) and call the device forms; or a resident alignment as
        (device address, n_seq, seq_len) with form "dev" or "packed".  fwd / rev: primer strings or packed words;
        forced: flags per primer (forward first), kept whatever they cover.  Returns (keep uint8[n], order, gains,
        covered uint8 (n_seq, P), covered_all, covered_kept)."""
        fn = {"host": self.L.msspe_panel_thin, "dev": self.L.msspe_panel_thin_dev,
              "packed": self.L.msspe_panel_thin_packed_dev}[form]
        return self._panel_thin(fn, (), genomes, opt, fwd, rev, max_mismatches, exact_3p, min_gain, forced, form)

    def panel_thin_thal(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, chem: Chem, mode,
                        tm_threshold: float, min_gain: int = 1, forced=None, form: str = "host"):
        """panel_thin over the segments a primer HOLDS: a match within max_mismatches (last exact_3p bases exact)
        counts when its thal score against the strand the primer anneals to is stable at tm_threshold
        (msspe_panel_thin_thal*; mode "any" (1) or "end1" (2), the rule of segment_coverage_thal).  Arguments and
        the returned tuple as panel_thin; covered marks the segments the kept set holds."""
        fn = {"host": self.L.msspe_panel_thin_thal, "dev": self.L.msspe_panel_thin_thal_dev,
              "packed": self.L.msspe_panel_thin_thal_packed_dev}[form]
        return self._panel_thin(fn, (C.byref(chem), self._thal_mode(mode), tm_threshold), genomes, opt, fwd, rev,
                                max_mismatches, exact_3p, min_gain, forced, form)

    # ---- a panel thinned to a coverage depth (engine extension; msspe_panel_thin_depth*) -------------------------
    def panel_thin_depth(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, depth: int,
                         min_gain: int = 1, forced=None, form: str = "host"):
        """panel_thin to a depth: every segment keeps min(depth, primers it has) primers, a word listed twice in a
        direction counting once (msspe_panel_thin_depth*).  Arguments as panel_thin.  Returns (keep uint8[n], order,
        gains, depth_all uint8 (n_seq, P), depth_kept uint8 (n_seq, P), counts int64[4])."""
        fn = {"host": self.L.msspe_panel_thin_depth, "dev": self.L.msspe_panel_thin_depth_dev,
              "packed": self.L.msspe_panel_thin_depth_packed_dev}[form]
        return self._panel_thin(fn, (), genomes, opt, fwd, rev, max_mismatches, exact_3p, min_gain, forced, form, depth)

    def panel_thin_thal_depth(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, chem: Chem,
                              mode, tm_threshold: float, depth: int, min_gain: int = 1, forced=None,
                              form: str = "host"):
        """panel_thin_depth over the segments a primer HOLDS (msspe_panel_thin_thal_depth*): arguments as
        panel_thin_thal plus depth, the returned tuple as panel_thin_depth."""
        fn = {"host": self.L.msspe_panel_thin_thal_depth, "dev": self.L.msspe_panel_thin_thal_depth_dev,
              "packed": self.L.msspe_panel_thin_thal_depth_packed_dev}[form]
        return self._panel_thin(fn, (C.byref(chem), self._thal_mode(mode), tm_threshold), genomes, opt, fwd, rev,
                                max_mismatches, exact_3p, min_gain, forced, form, depth)

    @staticmethod
    def _segment_weights(weights, n_seg: int) -> np.ndarray:
        w = np.asarray(weights)
        if w.size != n_seg:
            raise ValueError("weights needs one entry per segment (n_seq * P)")
        if w.size and (w.min() < 0 or w.max() > 0xFFFFFFFF):
            raise ValueError("a weight must fit a uint32")
        return np.ascontiguousarray(w.reshape(-1), dtype=np.uint32)

    def panel_thin_weighted(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, weights,
                            min_gain: int = 1, forced=None, form: str = "host"):
        """panel_thin on a weight per segment (msspe_panel_thin_weighted*): a gain is the sum of weights over the new
        segments, min_gain is in weight units.  weights: n_seq * P non-negative integers (any shape), their total at
        most 2^32 - 1.  Arguments and forms as panel_thin.  Returns (keep uint8[n], order, gains, covered uint8
        (n_seq, P), covered_all, covered_kept, weight_all, weight_kept)."""
        fn = {"host": self.L.msspe_panel_thin_weighted, "dev": self.L.msspe_panel_thin_weighted_dev,
              "packed": self.L.msspe_panel_thin_weighted_packed_dev}[form]
        return self._panel_thin(fn, (), genomes, opt, fwd, rev, max_mismatches, exact_3p, min_gain, forced, form,
                                weights=weights)

    @staticmethod
    def _primer_costs(costs, n: int) -> np.ndarray:
        c = np.asarray(costs)
        if c.shape != (n,):
            raise ValueError("costs needs one entry per primer (forward list, then reverse list)")
        if c.size and (c.min() < 0 or c.max() > 0xFFFFFFFF):
            raise ValueError("a cost must fit a uint32")
        return np.ascontiguousarray(c, dtype=np.uint32)

    def panel_thin_cost(self, genomes, opt: KmerOpt, fwd, rev, max_mismatches: int, exact_3p: int, costs, weights=None,
                        min_gain: int = 1, forced=None, form: str = "host"):
        """panel_thin by gain per cost (msspe_panel_thin_cost*): a round keeps the primer of greatest gain / cost among
        those whose gain reaches min_gain, compared exactly (equal ratios: the greater gain, then the lowest index).
        costs: one integer 1 .. 2^32 - 1 per primer, forward list then reverse list.  weights: as panel_thin_weighted,
        or None for a count of segments.  Arguments and forms as panel_thin.  Returns panel_thin_weighted's tuple plus
        cost_all, cost_kept (without weights the two weights are the two covered counts)."""
        fn = {"host": self.L.msspe_panel_thin_cost, "dev": self.L.msspe_panel_thin_cost_dev,
              "packed": self.L.msspe_panel_thin_cost_packed_dev}[form]
        return self._panel_thin(fn, (), genomes, opt, fwd, rev, max_mismatches, exact_3p, min_gain, forced, form,
                                weights=weights, costs=costs)

    def _panel_thin(self, fn, scoring, genomes, opt, fwd, rev, max_mismatches, exact_3p, min_gain, forced, form,
                    depth=None, weights=None, costs=None):
        owned = None
        if isinstance(genomes, tuple):
            if form == "host":
                raise ValueError("a resident alignment needs form='dev' or 'packed'")
            handle, n_seq, seq_len = genomes
            seqs_arg = C.c_void_p(handle)
        else:
            a = np.ascontiguousarray(genomes, dtype=np.uint8)
            n_seq, seq_len = a.shape
            if form == "host":
                seqs_arg = a.ctypes.data
            elif form == "packed":
                owned = self.put_rows_packed(a)
                seqs_arg = C.c_void_p(owned)
            else:
                dev = C.c_void_p()
                self._check(self.L.msspe_device_put(self.ptr, a.ctypes.data, a.size, C.byref(dev)))
                owned = int(dev.value)
                seqs_arg = C.c_void_p(owned)
        try:
            P = 0 if seq_len < opt.segment_size else (seq_len - opt.segment_size) // opt.overlap_size + 1
            f, r = _words(fwd), _words(rev)
            n = len(f) + len(r)
            flags = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
            if flags is not None and flags.shape != (n,):
                raise ValueError("forced needs one flag per primer")
            keep = np.zeros(n, dtype=np.uint8)
            order = np.zeros(max(n, 1), dtype=np.uint32)
            gains = np.zeros(max(n, 1), dtype=np.uint32)
            covered = np.zeros((n_seq, P), dtype=np.uint8)
            n_picked, c_all, c_kept = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
            mm = MismatchOpt(max_mismatches, exact_3p)
            extra_in = ()
            if costs is not None:
                w = None if weights is None else self._segment_weights(weights, n_seq * P)
                c = self._primer_costs(costs, n)
                w_all, w_kept, k_all, k_kept = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
                thin = ThinOpt(min_gain)
                extra_in = (None if w is None else w.ctypes.data, c.ctypes.data)
                outs = (covered.ctypes.data, C.byref(c_all), C.byref(c_kept), C.byref(w_all), C.byref(w_kept),
                        C.byref(k_all), C.byref(k_kept))
            elif weights is not None:
                w = self._segment_weights(weights, n_seq * P)
                w_all, w_kept = C.c_uint64(0), C.c_uint64(0)
                thin = ThinOpt(min_gain)
                extra_in = (w.ctypes.data,)
                outs = (covered.ctypes.data, C.byref(c_all), C.byref(c_kept), C.byref(w_all), C.byref(w_kept))
            elif depth is None:
                thin = ThinOpt(min_gain)
                outs = (covered.ctypes.data, C.byref(c_all), C.byref(c_kept))
            else:
                thin = ThinDepthOpt(min_gain, depth)
                depth_kept = np.zeros((n_seq, P), dtype=np.uint8)
                counts = (C.c_longlong * 4)()
                outs = (covered.ctypes.data, depth_kept.ctypes.data, counts)
            self._check(fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), C.byref(mm), C.byref(thin), *scoring,
                           f.ctypes.data, len(f), r.ctypes.data, len(r),
                           flags.ctypes.data if flags is not None else None, *extra_in, keep.ctypes.data,
                           order.ctypes.data, gains.ctypes.data, C.byref(n_picked), *outs))
        finally:
            if owned is not None:
                self.device_free(owned)
        if costs is not None:
            return (keep, order[:n_picked.value].copy(), gains[:n_picked.value].copy(), covered, int(c_all.value),
                    int(c_kept.value), int(w_all.value), int(w_kept.value), int(k_all.value), int(k_kept.value))
        if weights is not None:
            return (keep, order[:n_picked.value].copy(), gains[:n_picked.value].copy(), covered, int(c_all.value),
                    int(c_kept.value), int(w_all.value), int(w_kept.value))
        if depth is not None:
            return (keep, order[:n_picked.value].copy(), gains[:n_picked.value].copy(), covered, depth_kept,
                    np.array(list(counts), dtype=np.int64))
        return (keep, order[:n_picked.value].copy(), gains[:n_picked.value].copy(), covered, int(c_all.value),
                int(c_kept.value))

    # ---- a conflict-free panel selected by coverage (engine extension; msspe_panel_select*) ----------------------
    def panel_select(self, genomes, opt: KmerOpt, fwd, rev, rule: SeedRule, bitmap=None, max_tubes: int = 1,
                     min_gain: int = 1, drop_self_pairs: bool = False, forced=None, form: str = "bitmap",
                     chem: Chem | None = None, threshold: float = -9000.0, end_tm_threshold: float | None = None):
        """Greedy set cover in which a pick bars its conflict neighbours from its tube (msspe_panel_select*).
        genomes, fwd, rev, forced as panel_thin; rule: seed_rule(M, E[, mode, chem, tm]) says what a primer covers.
        form "bitmap": `bitmap` is a host uint64 (n, ceil(n/64)) array (the layout of cross_dimer_dev over the pool
        forward words then reverse words) and the alignment goes over from the host; "dev" / "packed": the alignment is
        uploaded (as bytes / packed rows) or resident as (device address, n_seq, seq_len), and `bitmap` is either such
        an array (uploaded for the call) or a device address; "screen": the call screens the pool itself at `chem`
        (default Chem.ntthal()) and `threshold`, with end_tm_threshold under the rule (ANY at threshold, END at
        end_tm_threshold; msspe_panel_select_rule).  Returns a dict: keep, order, gains, tube, barred (uint8[n]), covered
        (n_seq, P), covered_all, covered_kept, tubes_used."""
        return self._panel_select(None, genomes, opt, fwd, rev, rule, bitmap, max_tubes, min_gain, drop_self_pairs,
                                  forced, form, chem, threshold, end_tm_threshold)

    def panel_select_weighted(self, genomes, opt: KmerOpt, fwd, rev, rule: SeedRule, weights, bitmap=None,
                              max_tubes: int = 1, min_gain: int = 1, drop_self_pairs: bool = False, forced=None,
                              form: str = "dev", chem: Chem | None = None, threshold: float | None = -9000.0,
                              end_tm_threshold: float | None = None):
        """panel_select on a weight per segment (msspe_panel_select_weighted*): a gain is the sum of weights over the
        new segments, min_gain is in weight units.  weights: n_seq * P non-negative integers (any shape), their total
        at most 2^32 - 1.  Arguments as panel_select; form "dev" / "packed" (bitmap: a host array or a device address)
        or "screen" (msspe_panel_select_weighted_rule: ANY at threshold, END at end_tm_threshold, either may be None).
        Returns panel_select's dict plus weight_all and weight_kept."""
        if form not in ("dev", "packed", "screen"):
            raise ValueError("form must be 'dev', 'packed' or 'screen'")
        return self._panel_select(None, genomes, opt, fwd, rev, rule, bitmap, max_tubes, min_gain, drop_self_pairs,
                                  forced, form, chem, threshold, end_tm_threshold, weights=weights)

    def panel_select_cost(self, genomes, opt: KmerOpt, fwd, rev, rule: SeedRule, costs, weights=None, bitmap=None,
                          max_tubes: int = 1, min_gain: int = 1, drop_self_pairs: bool = False, forced=None,
                          form: str = "dev", chem: Chem | None = None, threshold: float | None = -9000.0,
                          end_tm_threshold: float | None = None):
        """panel_select by gain per cost (msspe_panel_select_cost*): a round keeps the live primer of greatest gain /
        cost among those whose gain reaches min_gain, compared exactly (equal ratios: the greater gain, then the
        lowest index).  costs: one integer 1 .. 2^32 - 1 per primer, forward list then reverse list.  weights: as
        panel_select_weighted, or None for a count of segments.  Arguments and forms as panel_select_weighted.  Returns
        its dict plus cost_all and cost_kept (without weights the two weights are the two covered counts)."""
        if form not in ("dev", "packed", "screen"):
            raise ValueError("form must be 'dev', 'packed' or 'screen'")
        return self._panel_select(None, genomes, opt, fwd, rev, rule, bitmap, max_tubes, min_gain, drop_self_pairs,
                                  forced, form, chem, threshold, end_tm_threshold, weights=weights, costs=costs)

    def _panel_select(self, _depth, genomes, opt, fwd, rev, rule, bitmap, max_tubes, min_gain, drop_self_pairs, forced,
                      form, chem, threshold, end_tm_threshold, weights=None, costs=None):
        """panel_select (_depth None) and panel_select_depth: the same inputs, the calls' own outputs; with weights,
        panel_select_weighted; with costs, panel_select_cost."""
        if form not in ("bitmap", "dev", "packed", "screen"):
            raise ValueError("form must be 'bitmap', 'dev', 'packed' or 'screen'")
        f, r = _words(fwd), _words(rev)
        n = len(f) + len(r)
        owned = []
        try:
            if isinstance(genomes, tuple):
                if form in ("bitmap", "screen"):
                    raise ValueError("a resident alignment needs form='dev' or 'packed'")
                handle, n_seq, seq_len = genomes
                seqs_arg = C.c_void_p(handle)
            else:
                a = np.ascontiguousarray(genomes, dtype=np.uint8)
                n_seq, seq_len = a.shape
                if form in ("bitmap", "screen"):
                    seqs_arg = a.ctypes.data
                elif form == "packed":
                    owned.append(self.put_rows_packed(a))
                    seqs_arg = C.c_void_p(owned[-1])
                else:
                    dev = C.c_void_p()
                    self._check(self.L.msspe_device_put(self.ptr, a.ctypes.data, a.size, C.byref(dev)))
                    owned.append(int(dev.value))
                    seqs_arg = C.c_void_p(owned[-1])
            if form == "screen":
                chem = chem or Chem.ntthal()
                if end_tm_threshold is not None or weights is not None or costs is not None:   # these take the rule only
                    conflict_rule = ConflictRule.of(threshold, end_tm_threshold)
                    graph = (C.byref(chem), C.byref(conflict_rule))
                elif threshold is None:
                    raise ValueError("form='screen' needs a threshold, an end_tm_threshold or both")
                else:
                    graph = (C.byref(chem), C.c_float(threshold))
            elif isinstance(bitmap, (int, np.integer)) and form != "bitmap":
                graph = (C.c_void_p(int(bitmap)),)
            else:
                B = np.ascontiguousarray(bitmap, dtype=np.uint64) if bitmap is not None else np.zeros((n, (n + 63) // 64), np.uint64)
                if B.size != n * ((n + 63) // 64):
                    raise ValueError("bitmap needs n x ceil(n/64) words")
                if form == "bitmap":
                    graph = (B.ctypes.data if B.size else None,)
                else:
                    dev = C.c_void_p()
                    self._check(self.L.msspe_device_put(self.ptr, B.ctypes.data if B.size else None, B.nbytes,
                                                        C.byref(dev)))
                    owned.append(int(dev.value))
                    graph = (C.c_void_p(owned[-1]),)
            fn = {"bitmap": self.L.msspe_panel_select_bitmap, "dev": self.L.msspe_panel_select_dev,
                  "packed": self.L.msspe_panel_select_packed_dev, "screen": self.L.msspe_panel_select}[form]
            if form == "screen" and end_tm_threshold is not None:
                fn = self.L.msspe_panel_select_rule
            if _depth is not None:
                fn = getattr(self.L, fn.__name__.replace("msspe_panel_select", "msspe_panel_select_depth"))
            if weights is not None:
                fn = {"dev": self.L.msspe_panel_select_weighted_dev, "packed": self.L.msspe_panel_select_weighted_packed_dev,
                      "screen": self.L.msspe_panel_select_weighted_rule}[form]
            if costs is not None:
                fn = {"dev": self.L.msspe_panel_select_cost_dev, "packed": self.L.msspe_panel_select_cost_packed_dev,
                      "screen": self.L.msspe_panel_select_cost_rule}[form]
            P = 0 if seq_len < opt.segment_size else (seq_len - opt.segment_size) // opt.overlap_size + 1
            flags = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
            if flags is not None and flags.shape != (n,):
                raise ValueError("forced needs one flag per primer")
            keep = np.zeros(n, dtype=np.uint8)
            order = np.zeros(max(n, 1), dtype=np.uint32)
            gains = np.zeros(max(n, 1), dtype=np.uint32)
            tube = np.zeros(max(n, 1), dtype=np.uint8)
            barred = np.zeros(max(n, 1), dtype=np.uint8)
            covered = np.zeros((n_seq, P), dtype=np.uint8)
            n_picked, used, c_all, c_kept = C.c_int(0), C.c_int(0), C.c_longlong(0), C.c_longlong(0)
            if _depth is not None:
                layer = np.zeros(max(n, 1), dtype=np.uint8)
                depth_all = np.zeros((n_seq, P), dtype=np.uint8)
                depth_kept = np.zeros((n_seq, P), dtype=np.uint8)
                counts = (C.c_longlong * 4)()
                dsel = SelectDepthOpt(min_gain, max_tubes, 1 if drop_self_pairs else 0, _depth)
                self._check(fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), C.byref(rule), C.byref(dsel),
                               f.ctypes.data, len(f), r.ctypes.data, len(r),
                               flags.ctypes.data if flags is not None else None, *graph, keep.ctypes.data,
                               order.ctypes.data, gains.ctypes.data, C.byref(n_picked), tube.ctypes.data,
                               barred.ctypes.data, C.byref(used), layer.ctypes.data, depth_all.ctypes.data,
                               depth_kept.ctypes.data, counts))
                return {"keep": keep, "order": order[:n_picked.value].copy(), "gains": gains[:n_picked.value].copy(),
                        "layer": layer[:n_picked.value].copy(), "tube": tube[:n].copy(), "barred": barred[:n].copy(),
                        "depth_all": depth_all, "depth_kept": depth_kept,
                        "counts": np.array(list(counts), dtype=np.int64), "tubes_used": int(used.value)}
            sel = SelectOpt(min_gain, max_tubes, 1 if drop_self_pairs else 0)
            extra_in, extra_out = (), ()
            if weights is not None:
                w = self._segment_weights(weights, n_seq * P)
                w_all, w_kept = C.c_uint64(0), C.c_uint64(0)
                extra_in, extra_out = (w.ctypes.data,), (C.byref(w_all), C.byref(w_kept))
            if costs is not None:
                c = self._primer_costs(costs, n)
                k_all, k_kept = C.c_uint64(0), C.c_uint64(0)
                if weights is None:
                    w_all, w_kept = C.c_uint64(0), C.c_uint64(0)
                    extra_in, extra_out = (None,), (C.byref(w_all), C.byref(w_kept))
                extra_in += (c.ctypes.data,)
                extra_out += (C.byref(k_all), C.byref(k_kept))
            self._check(fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), C.byref(rule), C.byref(sel),
                           f.ctypes.data, len(f), r.ctypes.data, len(r),
                           flags.ctypes.data if flags is not None else None, *graph, *extra_in, keep.ctypes.data,
                           order.ctypes.data, gains.ctypes.data, C.byref(n_picked), tube.ctypes.data,
                           barred.ctypes.data, covered.ctypes.data, C.byref(c_all), C.byref(c_kept), C.byref(used),
                           *extra_out))
        finally:
            for d in owned:
                self.device_free(d)
        if costs is not None:
            return {"keep": keep, "order": order[:n_picked.value].copy(), "gains": gains[:n_picked.value].copy(),
                    "tube": tube[:n].copy(), "barred": barred[:n].copy(), "covered": covered,
                    "covered_all": int(c_all.value), "covered_kept": int(c_kept.value), "tubes_used": int(used.value),
                    "weight_all": int(w_all.value), "weight_kept": int(w_kept.value),
                    "cost_all": int(k_all.value), "cost_kept": int(k_kept.value)}
        if weights is not None:
            return {"keep": keep, "order": order[:n_picked.value].copy(), "gains": gains[:n_picked.value].copy(),
                    "tube": tube[:n].copy(), "barred": barred[:n].copy(), "covered": covered,
                    "covered_all": int(c_all.value), "covered_kept": int(c_kept.value), "tubes_used": int(used.value),
                    "weight_all": int(w_all.value), "weight_kept": int(w_kept.value)}
        return {"keep": keep, "order": order[:n_picked.value].copy(), "gains": gains[:n_picked.value].copy(),
                "tube": tube[:n].copy(), "barred": barred[:n].copy(), "covered": covered,
                "covered_all": int(c_all.value), "covered_kept": int(c_kept.value), "tubes_used": int(used.value)}

    def panel_select_depth(self, genomes, opt: KmerOpt, fwd, rev, rule: SeedRule, depth: int, bitmap=None,
                           max_tubes: int = 1, min_gain: int = 1, drop_self_pairs: bool = False, forced=None,
                           form: str = "bitmap", chem: Chem | None = None, threshold: float = -9000.0,
                           end_tm_threshold: float | None = None):
        """The selection to a coverage depth, layer by layer (msspe_panel_select_depth*): layer 1 is panel_select,
        layer r then adds primers for the segments that still have fewer than r, with the barring carried along.
        Arguments and forms as panel_select, plus depth (1..255).  Returns a dict: keep, order, gains, layer (the layer
        of every pick), tube, barred, depth_all, depth_kept (uint8 (n_seq, P), saturating at 255), counts (int64[4]:
        segments with depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >= depth), tubes_used."""
        return self._panel_select(int(depth), genomes, opt, fwd, rev, rule, bitmap, max_tubes, min_gain,
                                  drop_self_pairs, forced, form, chem, threshold, end_tm_threshold)

    # ---- off-target sites in a background ------------------------------------------------------
    @staticmethod
    def _records(records):
        recs = [r.encode() if isinstance(r, str) else bytes(r) for r in records]
        n = len(recs)
        ptrs = (C.c_char_p * max(n, 1))(*recs)
        lens = (C.c_size_t * max(n, 1))(*[len(r) for r in recs])
        return recs, ptrs, lens, n

    def put_stream_packed(self, records):
        """Upload a background (a list of str / bytes records of any lengths) as one packed stream, packed on the
        device behind the copy (msspe_device_put_stream_packed).  Returns (device address, total_len, record starts
        uint64); free the address with device_free()."""
        _recs, ptrs, lens, n = self._records(records)
        dev, total = C.c_void_p(), C.c_size_t(0)
        starts = np.zeros(n, dtype=np.uint64)
        self._check(self.L.msspe_device_put_stream_packed(self.ptr, ptrs, lens, n, C.byref(dev), C.byref(total),
                                                          starts.ctypes.data))
        return int(dev.value), int(total.value), starts

    def background_sites_packed(self, d_packed: int, total_len: int, primers, max_mismatches: int, exact_3p: int,
                                k: int | None = None, d_sites: int = 0, capacity: int = 0, d_count: int = 0):
        """Sites of each primer (strings, or packed uint64 words with k=) on a resident stream
        (msspe_background_sites_packed_dev).  Returns counts, uint64 (n, 2): [:, 0] plus strand, [:, 1] minus.
        d_sites / capacity / d_count: raw device addresses of a SITE_DTYPE list and its uint64 count (added to, the
        caller zeroes it); 0 = no list."""
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        mm = MismatchOpt(max_mismatches, exact_3p)
        self._check(self.L.msspe_background_sites_packed_dev(
            self.ptr, C.c_void_p(d_packed), total_len, k, C.byref(mm), w.ctypes.data, len(w), counts.ctypes.data,
            C.c_void_p(d_sites), capacity, C.c_void_p(d_count)))
        return counts

    def background_sites(self, records, primers, max_mismatches: int, exact_3p: int, k: int | None = None,
                         capacity: int | None = None):
        """Host form (msspe_background_sites): returns (counts, starts), or with a list capacity
        (counts, starts, sites) -- sites a SITE_DTYPE array sorted by (primer, strand, pos).  A capacity below the
        number of sites raises MsspeError (MSSPE_ERR_CAPACITY) carrying .count, .counts and the truncated .sites."""
        _recs, ptrs, lens, n = self._records(records)
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        starts = np.zeros(n, dtype=np.uint64)
        mm = MismatchOpt(max_mismatches, exact_3p)
        sites = np.zeros(max(capacity, 1), dtype=SITE_DTYPE) if capacity is not None else None
        count = C.c_uint64(0)
        rc = self.L.msspe_background_sites(
            self.ptr, ptrs, lens, n, k, C.byref(mm), w.ctypes.data, len(w), counts.ctypes.data,
            sites.ctypes.data if sites is not None else None, capacity or 0, C.byref(count), starts.ctypes.data)
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count, err.counts = int(count.value), counts
            err.sites = sites[:min(int(count.value), capacity or 0)] if sites is not None else None
            raise err
        if sites is None:
            return counts, starts
        return counts, starts, sites[:count.value]

    @staticmethod
    def _thal_mode(mode) -> int:
        return THAL_MODES[mode] if isinstance(mode, str) else int(mode)

    def background_thal_packed(self, d_packed: int, total_len: int, primers, max_mismatches: int, exact_3p: int,
                               chem: Chem, tm_threshold: float, mode="any", k: int | None = None, d_sites: int = 0,
                               capacity: int = 0, d_count: int = 0, flank: int = 0):
        """Sites of each primer on a resident stream, each scored with thal (msspe_background_thal_packed_dev): the
        primer against the strand it would anneal to, mode "any" (1) or "end1" (2); a site is stable iff
        round_fixed_f32(max(0, t), 2) >= tm_threshold.  Returns (counts, stable), uint64 (n, 2) each: [:, 0] plus
        strand, [:, 1] minus.  d_sites / capacity / d_count: raw device addresses of a SCORED_SITE_DTYPE list and its
        uint64 count (added to, the caller zeroes it); 0 = no list.  flank: the template oligo takes up to this many
        base columns on either side of the window (0..4, k + 2 flank <= 32; msspe_background_thal_flank_packed_dev);
        0 is the blunt window and calls the function without _flank."""
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        mm = MismatchOpt(max_mismatches, exact_3p)
        fn, extra = ((self.L.msspe_background_thal_flank_packed_dev, (flank,)) if flank else
                     (self.L.msspe_background_thal_packed_dev, ()))
        self._check(fn(
            self.ptr, C.c_void_p(d_packed), total_len, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem),
            self._thal_mode(mode), tm_threshold, *extra, counts.ctypes.data, stable.ctypes.data, C.c_void_p(d_sites),
            capacity, C.c_void_p(d_count)))
        return counts, stable

    def background_thal(self, records, primers, max_mismatches: int, exact_3p: int, chem: Chem, tm_threshold: float,
                        mode="any", k: int | None = None, capacity: int | None = None, flank: int = 0):
        """Host form (msspe_background_thal): returns (counts, stable, starts), or with a list capacity
        (counts, stable, starts, sites) -- sites a SCORED_SITE_DTYPE array sorted by (primer, strand, pos), one record
        per site, stable or not.  A capacity below the number of sites raises MsspeError (MSSPE_ERR_CAPACITY) carrying
        .count, .counts, .stable and the truncated .sites.  flank: as background_thal_packed
        (msspe_background_thal_flank when nonzero)."""
        _recs, ptrs, lens, n = self._records(records)
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        starts = np.zeros(n, dtype=np.uint64)
        mm = MismatchOpt(max_mismatches, exact_3p)
        sites = np.zeros(max(capacity, 1), dtype=SCORED_SITE_DTYPE) if capacity is not None else None
        count = C.c_uint64(0)
        fn, extra = ((self.L.msspe_background_thal_flank, (flank,)) if flank else (self.L.msspe_background_thal, ()))
        rc = fn(
            self.ptr, ptrs, lens, n, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem), self._thal_mode(mode),
            tm_threshold, *extra, counts.ctypes.data, stable.ctypes.data,
            sites.ctypes.data if sites is not None else None, capacity or 0, C.byref(count), starts.ctypes.data)
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count, err.counts, err.stable = int(count.value), counts, stable
            err.sites = sites[:min(int(count.value), capacity or 0)] if sites is not None else None
            raise err
        if sites is None:
            return counts, stable, starts
        return counts, stable, starts, sites[:count.value]

    def background_amplicons_packed(self, d_packed: int, total_len: int, primers, max_mismatches: int, exact_3p: int,
                                    chem: Chem, tm_threshold: float, mode, min_len: int, max_len: int,
                                    record_start=None, k: int | None = None, d_amplicons: int = 0, capacity: int = 0,
                                    d_count: int = 0, flank: int = 0):
        """Off-target amplicons on a resident stream (msspe_background_amplicons_packed_dev): pairs of stable sites, a
        plus-strand one at p and a minus-strand one at q >= p of the same record with min_len <= q + k - p <= max_len.
        record_start: the record starts put_stream_packed returned (None: the stream is one record).  Returns
        (counts, stable, amplicons, total): uint64 (n, 2) each -- sites and stable sites per strand, amplicons with
        the primer as forward [:, 0] and as reverse [:, 1] -- and the number of amplicons.  d_amplicons / capacity /
        d_count: raw device addresses of an AMPLICON_DTYPE list and its uint64 count (added to); 0 = no list.
        flank: the stable sites are those of background_thal_packed at this flank
        (msspe_background_amplicons_flank_packed_dev when nonzero)."""
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        amps = np.zeros((len(w), 2), dtype=np.uint64)
        total = C.c_uint64(0)
        mm, opt = MismatchOpt(max_mismatches, exact_3p), AmpliconOpt(min_len, max_len)
        starts = None if record_start is None else np.ascontiguousarray(record_start, dtype=np.uint64)
        fn, extra = ((self.L.msspe_background_amplicons_flank_packed_dev, (flank,)) if flank else
                     (self.L.msspe_background_amplicons_packed_dev, ()))
        self._check(fn(
            self.ptr, C.c_void_p(d_packed), total_len, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem),
            self._thal_mode(mode), tm_threshold, *extra, C.byref(opt), None if starts is None else starts.ctypes.data,
            0 if starts is None else len(starts), counts.ctypes.data, stable.ctypes.data, amps.ctypes.data,
            C.byref(total), C.c_void_p(d_amplicons), capacity, C.c_void_p(d_count)))
        return counts, stable, amps, int(total.value)

    def background_amplicons(self, records, primers, max_mismatches: int, exact_3p: int, chem: Chem,
                             tm_threshold: float, mode, min_len: int, max_len: int, k: int | None = None,
                             capacity: int | None = None, flank: int = 0):
        """Host form (msspe_background_amplicons): returns (counts, stable, amplicons, total, starts), or with a list
        capacity (..., starts, list) -- list an AMPLICON_DTYPE array sorted by (pos, len, fwd, rev).  A capacity below
        the number of amplicons raises MsspeError (MSSPE_ERR_CAPACITY) carrying .count, .counts, .stable, .amplicons,
        .total and the truncated .list.  flank: as background_amplicons_packed (msspe_background_amplicons_flank when
        nonzero)."""
        _recs, ptrs, lens, n = self._records(records)
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        amps = np.zeros((len(w), 2), dtype=np.uint64)
        starts = np.zeros(n, dtype=np.uint64)
        total, count = C.c_uint64(0), C.c_uint64(0)
        mm, opt = MismatchOpt(max_mismatches, exact_3p), AmpliconOpt(min_len, max_len)
        lst = np.zeros(max(capacity, 1), dtype=AMPLICON_DTYPE) if capacity is not None else None
        fn, extra = ((self.L.msspe_background_amplicons_flank, (flank,)) if flank else
                     (self.L.msspe_background_amplicons, ()))
        rc = fn(
            self.ptr, ptrs, lens, n, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem), self._thal_mode(mode),
            tm_threshold, *extra, C.byref(opt), counts.ctypes.data, stable.ctypes.data, amps.ctypes.data, C.byref(total),
            lst.ctypes.data if lst is not None else None, capacity or 0, C.byref(count), starts.ctypes.data)
        if rc:
            err = MsspeError(rc, self.L.msspe_last_error(self.ptr).decode())
            err.count, err.counts, err.stable, err.amplicons = int(count.value), counts, stable, amps
            err.total = int(total.value)
            err.list = lst[:min(int(count.value), capacity or 0)] if lst is not None else None
            raise err
        if lst is None:
            return counts, stable, amps, int(total.value), starts
        return counts, stable, amps, int(total.value), starts, lst[:count.value]

    def stream_reach_packed(self, d_packed: int, total_len: int, primers, max_mismatches: int, exact_3p: int,
                            chem: Chem, tm_threshold: float, mode, reach: int, record_start=None,
                            k: int | None = None, flank: int = 0):
        """What the stable sites of a resident stream reach (msspe_stream_reach_packed_dev): per record the columns
        within `reach` downstream of a stable plus-strand site (towards increasing positions) or minus-strand site
        (towards decreasing positions), and the longest run nothing reaches.  record_start: the record starts
        put_stream_packed returned (None: the stream is one record).  Returns (counts, stable, records): uint64
        (n, 2) each as background_thal_packed returns them, and a REACH_RECORD_DTYPE array, one entry per record."""
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        mm, opt = MismatchOpt(max_mismatches, exact_3p), ReachOpt(reach)
        starts = None if record_start is None else np.ascontiguousarray(record_start, dtype=np.uint64)
        recs = np.zeros(max(1 if starts is None else len(starts), 1), dtype=REACH_RECORD_DTYPE)
        self._check(self.L.msspe_stream_reach_packed_dev(
            self.ptr, C.c_void_p(d_packed), total_len, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem),
            self._thal_mode(mode), tm_threshold, flank, C.byref(opt), None if starts is None else starts.ctypes.data,
            0 if starts is None else len(starts), counts.ctypes.data, stable.ctypes.data, recs.ctypes.data))
        return counts, stable, recs[:1 if starts is None else len(starts)]

    def stream_reach(self, records, primers, max_mismatches: int, exact_3p: int, chem: Chem, tm_threshold: float,
                     mode, reach: int, k: int | None = None, flank: int = 0):
        """Host form (msspe_stream_reach): returns (counts, stable, records, starts)."""
        _recs, ptrs, lens, n = self._records(records)
        w, k = _words_k(primers, k)
        counts = np.zeros((len(w), 2), dtype=np.uint64)
        stable = np.zeros((len(w), 2), dtype=np.uint64)
        starts = np.zeros(n, dtype=np.uint64)
        mm, opt = MismatchOpt(max_mismatches, exact_3p), ReachOpt(reach)
        recs = np.zeros(max(n, 1), dtype=REACH_RECORD_DTYPE)
        self._check(self.L.msspe_stream_reach(
            self.ptr, ptrs, lens, n, k, C.byref(mm), w.ctypes.data, len(w), C.byref(chem), self._thal_mode(mode),
            tm_threshold, flank, C.byref(opt), counts.ctypes.data, stable.ctypes.data, recs.ctypes.data,
            starts.ctypes.data))
        return counts, stable, recs[:n], starts

    # ---- a panel thinned on target reach (engine extension; msspe_panel_thin_reach*) -----------------------------
    @staticmethod
    def _thin_reach_out(n: int, forced):
        if forced is None:
            f = None
        else:
            f = np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
            if f.size != n:
                raise ValueError("forced needs one flag per primer")
        return (f, np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32),
                np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32), C.c_int(0),
                C.c_longlong(0), C.c_longlong(0))

    def panel_thin_reach_packed(self, d_packed: int, total_len: int, primers, max_mismatches: int, exact_3p: int,
                                chem: Chem, tm_threshold: float, mode, reach: int, min_gain: int = 1, forced=None,
                                record_start=None, k: int | None = None, flank: int = 0, want_records: bool = True):
        """The primers a resident stream's reach needs (msspe_panel_thin_reach_packed_dev): a greedy set cover over
        the columns each primer's stable sites reach, forced primers first, ties to the lowest index, until the best
        gain falls below min_gain.  Arguments as stream_reach_packed.  Returns a dict: keep (uint8[n]), order, gains
        (the picks), primer_reach (uint32[n], |R_p|), reached_all, reached_kept, counts, stable (whole panel) and
        records (the kept panel's REACH_RECORD_DTYPE array; None with want_records False)."""
        w, k = _words_k(primers, k)
        n = len(w)
        counts = np.zeros((n, 2), dtype=np.uint64)
        stable = np.zeros((n, 2), dtype=np.uint64)
        mm, opt, thin = MismatchOpt(max_mismatches, exact_3p), ReachOpt(reach), ThinOpt(min_gain)
        starts = None if record_start is None else np.ascontiguousarray(record_start, dtype=np.uint64)
        nr = 1 if starts is None else len(starts)
        recs = np.zeros(max(nr, 1), dtype=REACH_RECORD_DTYPE) if want_records else None
        f, keep, order, gains, own, picked, r_all, r_kept = self._thin_reach_out(n, forced)
        self._check(self.L.msspe_panel_thin_reach_packed_dev(
            self.ptr, C.c_void_p(d_packed), total_len, k, C.byref(mm), w.ctypes.data, n, C.byref(chem),
            self._thal_mode(mode), tm_threshold, flank, C.byref(opt), C.byref(thin),
            None if f is None else f.ctypes.data, None if starts is None else starts.ctypes.data,
            0 if starts is None else len(starts), keep.ctypes.data, order.ctypes.data, gains.ctypes.data,
            C.byref(picked), own.ctypes.data, C.byref(r_all), C.byref(r_kept), counts.ctypes.data, stable.ctypes.data,
            None if recs is None else recs.ctypes.data))
        return {"keep": keep[:n], "order": order[:picked.value], "gains": gains[:picked.value],
                "primer_reach": own[:n], "reached_all": int(r_all.value), "reached_kept": int(r_kept.value),
                "counts": counts, "stable": stable, "records": None if recs is None else recs[:nr]}

    def panel_thin_reach(self, records, primers, max_mismatches: int, exact_3p: int, chem: Chem, tm_threshold: float,
                         mode, reach: int, min_gain: int = 1, forced=None, k: int | None = None, flank: int = 0,
                         want_records: bool = True):
        """Host form (msspe_panel_thin_reach): the dict of panel_thin_reach_packed, and starts."""
        _recs, ptrs, lens, nr = self._records(records)
        w, k = _words_k(primers, k)
        n = len(w)
        counts = np.zeros((n, 2), dtype=np.uint64)
        stable = np.zeros((n, 2), dtype=np.uint64)
        starts = np.zeros(nr, dtype=np.uint64)
        mm, opt, thin = MismatchOpt(max_mismatches, exact_3p), ReachOpt(reach), ThinOpt(min_gain)
        recs = np.zeros(max(nr, 1), dtype=REACH_RECORD_DTYPE) if want_records else None
        f, keep, order, gains, own, picked, r_all, r_kept = self._thin_reach_out(n, forced)
        self._check(self.L.msspe_panel_thin_reach(
            self.ptr, ptrs, lens, nr, k, C.byref(mm), w.ctypes.data, n, C.byref(chem), self._thal_mode(mode),
            tm_threshold, flank, C.byref(opt), C.byref(thin), None if f is None else f.ctypes.data, keep.ctypes.data,
            order.ctypes.data, gains.ctypes.data, C.byref(picked), own.ctypes.data, C.byref(r_all), C.byref(r_kept),
            counts.ctypes.data, stable.ctypes.data, None if recs is None else recs.ctypes.data, starts.ctypes.data))
        return {"keep": keep[:n], "order": order[:picked.value], "gains": gains[:picked.value],
                "primer_reach": own[:n], "reached_all": int(r_all.value), "reached_kept": int(r_kept.value),
                "counts": counts, "stable": stable, "records": None if recs is None else recs[:nr], "starts": starts}

    def thal_detail(self, a, b, chem: Chem | None = None, mode="any") -> np.ndarray:
        """Full thal record of the pairs (a[i], b[i]) (msspe_thal_detail_pairs): two equal-length lists of strings of
        one length; mode "any" (1) or "end1" (2).  Returns a THAL_DETAIL_DTYPE array, one record per pair: dS
        (salt-corrected), dH, dG, t, no_structure, n_pairs and the traced base pairs ps1 / ps2 (ps1[i-1] = 1-based
        partner in the REVERSED oligo 2, 0 = unpaired).  A record without a structure is all zero but no_structure."""
        a, b = list(a), list(b)
        k = len(a[0]) if a else 2          # an empty call's length does not matter
        if len(a) != len(b) or any(len(s) != k for s in a) or any(len(s) != k for s in b):
            raise MsspeError(1, "thal_detail needs two equal-length lists of oligos of one length")
        chem = chem or Chem.ntthal()
        out = np.zeros(len(a), dtype=THAL_DETAIL_DTYPE)
        self._check(self.L.msspe_thal_detail_pairs(self.ptr, "".join(a).encode(), "".join(b).encode(), len(a), k,
                                                   C.byref(chem), self._thal_mode(mode), out.ctypes.data))
        return out

    def pair_stage_samples(self):
        """[(row, col, reason bits)] for up to 1024 pairs the integer stage handed on."""
        v = (C.c_uint64 * 1024)()
        n = C.c_int(0)
        self._check(self.L.msspe_pair_stage_samples(self.ptr, v, 1024, C.byref(n)))
        return [(int(x >> 40), int((x >> 16) & 0xffffff), int(x & 0xffff)) for x in v[:n.value]]

    def pair_stage_stats(self) -> dict:
        """Diagnostics of the exact-integer stages since the last call (resets them): the
        matrix-mode kernel's counts at the top level, the list-mode kernel's under "list";
        "needed_f64" = pairs only the f64 kernels could answer."""
        v = (C.c_uint64 * 16)()
        self._check(self.L.msspe_pair_stage_stats(self.ptr, v))
        names = ("deferred", "tm_near_tie", "loop_eq_value", "loop_tie", "rejected_min", "pick_tie",
                 "replay_mismatch", "path_tie")
        out = {n: int(v[i]) for i, n in enumerate(names)}
        out["list"] = {n: int(v[8 + i]) for i, n in enumerate(names)}
        out["needed_f64"] = int(v[8])
        # pairs the bound first stage (option pair_bound) could not cull and handed to list 0; not part of "deferred"
        out["bound_survivors"] = self.info("bound_survivors")
        # ordered pairs a mirrored bound stage (option pair_mirror) answered or handed on without a fill of their own
        out["bound_mirrored"] = self.info("bound_mirrored")
        # the bound list stage (option pair_bound_list): entries of list U (unordered pairs under the mirror), and the
        # ordered pairs it could not cull and appended to list 0
        out["bound_list_pairs"] = self.info("bound_list_pairs")
        out["bound_list_survivors"] = self.info("bound_list_survivors")
        # ordered pairs the windowed first stage (option pair_bound_window) could not cull and sent to list U
        out["bound_window_survivors"] = self.info("bound_window_survivors")
        return out

    # ---- stage B ---------------------------------------------------------------------------
    def oligo_stats(self, pool, chem: Chem | None = None):
        buf, n, k = _ascii(pool)
        chem = chem or Chem.primer3()
        out = {name: np.empty(n) for name in ("tm", "gc", "self_any", "self_end", "hairpin")}
        self._check(self.L.msspe_oligo_stats(self.ptr, buf, n, k, C.byref(chem),
                                             *[out[x].ctypes.data for x in out]))
        return out

    def oligo_stats_dev(self, d_pool: int, n: int, k: int, chem: Chem, d_tm: int = 0, d_gc: int = 0,
                        d_self_any: int = 0, d_self_end: int = 0, d_hairpin: int = 0):
        """Device-pointer call (raw addresses of n packed oligos and of n doubles per requested statistic,
        0 = not wanted); asynchronous on the context's stream."""
        self._check(self.L.msspe_oligo_stats_dev(self.ptr, C.c_void_p(d_pool), n, k, C.byref(chem),
                                                 *[C.c_void_p(x) for x in (d_tm, d_gc, d_self_any, d_self_end, d_hairpin)]))

    # ---- stage A ---------------------------------------------------------------------------
    def kmer_candidates(self, seqs: np.ndarray, opt: KmerOpt, direction: int,
                        device_ptr: int | None = None, n_seq: int | None = None,
                        seq_len: int | None = None, capacity: int | None = None, *, seed=None, exclude=None):
        """seqs: uint8 (n_seq, L) host array (or pass device_ptr + shape).  Returns (words, freqs).
        capacity: size of the output buffers (default: max_iterations, which always suffices).
        seed: words (strings of length kmer_size, in the direction's key space) taken as already picked
        (msspe_kmer_candidates_seeded; host sequences only).
        exclude: words of the same form that must never be picked (msspe_kmer_candidates_sets; host sequences only)."""
        cap = max(1, opt.max_iterations if capacity is None else capacity)
        words = np.zeros(cap, dtype=np.uint64)
        freqs = np.zeros(cap, dtype=np.uint32)
        n_out = C.c_int(0)
        sw = _seed_words(seed, opt.kmer_size)
        xw = _seed_words(exclude, opt.kmer_size, "exclude")
        if xw is not None:
            if device_ptr is not None:
                raise ValueError("exclude= needs host sequences (or kmer_candidates_packed on a packed alignment)")
            a = np.ascontiguousarray(seqs, dtype=np.uint8)
            n_seq, seq_len = a.shape
            sets = _kmer_sets(sw, xw)
            self._check(self.L.msspe_kmer_candidates_sets(
                self.ptr, a.ctypes.data, n_seq, seq_len, C.byref(opt), direction, C.byref(sets),
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        elif sw is not None:
            if device_ptr is not None:
                raise ValueError("seed= needs host sequences (or kmer_candidates_packed on a packed alignment)")
            a = np.ascontiguousarray(seqs, dtype=np.uint8)
            n_seq, seq_len = a.shape
            self._check(self.L.msspe_kmer_candidates_seeded(
                self.ptr, a.ctypes.data, n_seq, seq_len, C.byref(opt), direction, sw.ctypes.data, len(sw),
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        elif device_ptr is None:
            a = np.ascontiguousarray(seqs, dtype=np.uint8)
            n_seq, seq_len = a.shape
            self._check(self.L.msspe_kmer_candidates(
                self.ptr, a.ctypes.data, n_seq, seq_len, C.byref(opt), direction,
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        else:
            self._check(self.L.msspe_kmer_candidates_dev(
                self.ptr, C.c_void_p(device_ptr), n_seq, seq_len, C.byref(opt), direction,
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        m = n_out.value
        return [unpack_oligo(w, opt.kmer_size) for w in words[:m]], freqs[:m].copy()

    def put_rows_packed(self, seqs: np.ndarray) -> int:
        """Upload an alignment (uint8 (n_seq, L)) in its compact device form (2-bit bases + validity bit, packed on
        the device behind the copy: msspe_device_put_rows_packed).  Returns the device address; free it with
        device_free()."""
        a = np.ascontiguousarray(seqs, dtype=np.uint8)
        n_seq, seq_len = a.shape
        ptrs = (C.c_char_p * n_seq)(*[C.cast(a[i].ctypes.data, C.c_char_p) for i in range(n_seq)])
        lens = (C.c_size_t * n_seq)(*([seq_len] * n_seq))
        dev = C.c_void_p()
        self._check(self.L.msspe_device_put_rows_packed(self.ptr, ptrs, lens, n_seq, seq_len, C.byref(dev)))
        return int(dev.value)

    def device_get(self, device_ptr: int, nbytes: int) -> np.ndarray:
        """nbytes bytes at a device address, behind everything queued on the engine's stream (msspe_device_get)."""
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self.L.msspe_device_get(self.ptr, C.c_void_p(device_ptr), nbytes, out.ctypes.data))
        return out

    def device_free(self, device_ptr: int) -> None:
        self._check(self.L.msspe_device_free(self.ptr, C.c_void_p(device_ptr)))

    def kmer_candidates_packed(self, d_packed: int, n_seq: int, seq_len: int, opt: KmerOpt, direction: int,
                               capacity: int | None = None, *, seed=None, exclude=None):
        """Stage A on a packed alignment resident on the device (put_rows_packed).  Returns (words, freqs).
        seed: as for kmer_candidates (msspe_kmer_candidates_seeded_packed_dev); exclude: words that must never be
        picked (msspe_kmer_candidates_sets_packed_dev)."""
        cap = max(1, opt.max_iterations if capacity is None else capacity)
        words = np.zeros(cap, dtype=np.uint64)
        freqs = np.zeros(cap, dtype=np.uint32)
        n_out = C.c_int(0)
        sw = _seed_words(seed, opt.kmer_size)
        xw = _seed_words(exclude, opt.kmer_size, "exclude")
        if xw is not None:
            sets = _kmer_sets(sw, xw)
            self._check(self.L.msspe_kmer_candidates_sets_packed_dev(
                self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), direction, C.byref(sets),
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        elif sw is not None:
            self._check(self.L.msspe_kmer_candidates_seeded_packed_dev(
                self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), direction, sw.ctypes.data, len(sw),
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        else:
            self._check(self.L.msspe_kmer_candidates_packed_dev(
                self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), direction,
                words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out)))
        m = n_out.value
        return [unpack_oligo(w, opt.kmer_size) for w in words[:m]], freqs[:m].copy()

    # ---- stage A seeded on what a panel covers (msspe_kmer_candidates_tolerant*) -------------------------------
    def _tolerant(self, fn, seqs_arg, n_seq, seq_len, opt, direction, seed, rule, exclude, capacity):
        cap = max(1, opt.max_iterations if capacity is None else capacity)
        words = np.zeros(cap, dtype=np.uint64)
        freqs = np.zeros(cap, dtype=np.uint32)
        n_out = C.c_int(0)
        P = (seq_len - opt.segment_size) // opt.overlap_size + 1 if seq_len >= opt.segment_size > 0 < opt.overlap_size else 0
        covered = np.zeros(max(0, n_seq) * P, dtype=np.uint8)
        parts = np.zeros(P, dtype=np.uint32)
        sw = _seed_words(seed, opt.kmer_size)
        xw = _seed_words(exclude, opt.kmer_size, "exclude")
        sets = _kmer_sets(sw, xw)
        self._check(fn(self.ptr, seqs_arg, n_seq, seq_len, C.byref(opt), direction, C.byref(sets), C.byref(rule),
                       words.ctypes.data, freqs.ctypes.data, cap, C.byref(n_out), covered.ctypes.data,
                       parts.ctypes.data))
        m = n_out.value
        return ([unpack_oligo(w, opt.kmer_size) for w in words[:m]], freqs[:m].copy(), covered.reshape(max(0, n_seq), P),
                parts)

    def kmer_candidates_tolerant(self, seqs: np.ndarray, opt: KmerOpt, direction: int, seed, rule: SeedRule, *,
                                 exclude=None, capacity: int | None = None):
        """Stage A extending a panel on what the panel covers (msspe_kmer_candidates_tolerant; host sequences): the
        seed words cover every segment of the direction they match under `rule` (seed_rule()).  Returns (words, freqs,
        seed_covered uint8 (n_seq, P), seed_partitions uint32 (P)): the winners, and the state before the first
        iteration."""
        a = np.ascontiguousarray(seqs, dtype=np.uint8)
        return self._tolerant(self.L.msspe_kmer_candidates_tolerant, a.ctypes.data, a.shape[0], a.shape[1], opt,
                              direction, seed, rule, exclude, capacity)

    def kmer_candidates_tolerant_packed(self, d_packed: int, n_seq: int, seq_len: int, opt: KmerOpt, direction: int,
                                        seed, rule: SeedRule, *, exclude=None, capacity: int | None = None):
        """The same on a packed alignment resident on the device (msspe_kmer_candidates_tolerant_packed_dev)."""
        return self._tolerant(self.L.msspe_kmer_candidates_tolerant_packed_dev, C.c_void_p(d_packed), n_seq, seq_len,
                              opt, direction, seed, rule, exclude, capacity)

    def kmer_candidates_tolerant_both_packed(self, d_packed: int, n_seq: int, seq_len: int, opt: KmerOpt, seed_fwd,
                                             seed_rev, rule: SeedRule, *, exclude_fwd=None, exclude_rev=None,
                                             capacity: int | None = None):
        """Both directions at once under one rule (msspe_kmer_candidates_both_tolerant_packed_dev): the two seeding
        passes one after the other, the two greedy loops side by side.  Returns the two directions' 4-tuples."""
        cap = max(1, opt.max_iterations if capacity is None else capacity)
        P = (seq_len - opt.segment_size) // opt.overlap_size + 1 if seq_len >= opt.segment_size > 0 < opt.overlap_size else 0
        w = [np.zeros(cap, dtype=np.uint64) for _ in range(2)]
        f = [np.zeros(cap, dtype=np.uint32) for _ in range(2)]
        cov = [np.zeros(max(0, n_seq) * P, dtype=np.uint8) for _ in range(2)]
        parts = [np.zeros(P, dtype=np.uint32) for _ in range(2)]
        n = [C.c_int(0), C.c_int(0)]
        lists = [(_seed_words(seed_fwd, opt.kmer_size), _seed_words(exclude_fwd, opt.kmer_size, "exclude")),
                 (_seed_words(seed_rev, opt.kmer_size), _seed_words(exclude_rev, opt.kmer_size, "exclude"))]
        sets = [_kmer_sets(*lists[0]), _kmer_sets(*lists[1])]
        self._check(self.L.msspe_kmer_candidates_both_tolerant_packed_dev(
            self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), C.byref(sets[0]), C.byref(sets[1]),
            C.byref(rule), w[0].ctypes.data, f[0].ctypes.data, C.byref(n[0]), w[1].ctypes.data, f[1].ctypes.data,
            C.byref(n[1]), cap, cov[0].ctypes.data, parts[0].ctypes.data, cov[1].ctypes.data, parts[1].ctypes.data))
        return tuple(([unpack_oligo(x, opt.kmer_size) for x in w[d][:n[d].value]], f[d][:n[d].value].copy(),
                      cov[d].reshape(max(0, n_seq), P), parts[d]) for d in (0, 1))



def _both(self, d_packed: int, n_seq: int, seq_len: int, opt: KmerOpt, capacity: int | None = None, *,
          seed_fwd=None, seed_rev=None, exclude_fwd=None, exclude_rev=None):
    """Stage A, both directions of a packed alignment at once (msspe_kmer_candidates_both_packed_dev).
    Returns ((words, freqs) of direction 0, (words, freqs) of direction 1).  seed_fwd / seed_rev: each direction's
    seed words, as for kmer_candidates (msspe_kmer_candidates_both_seeded_packed_dev); exclude_fwd / exclude_rev: each
    direction's words that must never be picked (msspe_kmer_candidates_both_sets_packed_dev)."""
    cap = max(1, opt.max_iterations if capacity is None else capacity)
    w = [np.zeros(cap, dtype=np.uint64) for _ in range(2)]
    f = [np.zeros(cap, dtype=np.uint32) for _ in range(2)]
    n = [C.c_int(0), C.c_int(0)]
    sf, sr = _seed_words(seed_fwd, opt.kmer_size), _seed_words(seed_rev, opt.kmer_size)
    xf, xr = _seed_words(exclude_fwd, opt.kmer_size, "exclude"), _seed_words(exclude_rev, opt.kmer_size, "exclude")
    if xf is not None or xr is not None:
        sets_f, sets_r = _kmer_sets(sf, xf), _kmer_sets(sr, xr)
        self._check(self.L.msspe_kmer_candidates_both_sets_packed_dev(
            self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), C.byref(sets_f), C.byref(sets_r),
            w[0].ctypes.data, f[0].ctypes.data, C.byref(n[0]), w[1].ctypes.data, f[1].ctypes.data, C.byref(n[1]), cap))
    elif sf is not None or sr is not None:
        sf = np.zeros(0, dtype=np.uint64) if sf is None else sf
        sr = np.zeros(0, dtype=np.uint64) if sr is None else sr
        self._check(self.L.msspe_kmer_candidates_both_seeded_packed_dev(
            self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), sf.ctypes.data, len(sf), sr.ctypes.data,
            len(sr), w[0].ctypes.data, f[0].ctypes.data, C.byref(n[0]), w[1].ctypes.data, f[1].ctypes.data,
            C.byref(n[1]), cap))
    else:
        self._check(self.L.msspe_kmer_candidates_both_packed_dev(
            self.ptr, C.c_void_p(d_packed), n_seq, seq_len, C.byref(opt), w[0].ctypes.data, f[0].ctypes.data,
            C.byref(n[0]), w[1].ctypes.data, f[1].ctypes.data, C.byref(n[1]), cap))
    return tuple(([unpack_oligo(x, opt.kmer_size) for x in w[d][:n[d].value]], f[d][:n[d].value].copy()) for d in (0, 1))


Engine.kmer_candidates_both_packed = _both


def group_rows(n: int, n_members: int, member: int) -> np.ndarray:
    """Pool rows a member of a group screens (include/msspe_hip.h msspe_group_rows; host only)."""
    L = load_library()
    cnt = C.c_int(0)
    rc = L.msspe_group_rows(n, n_members, member, None, 0, C.byref(cnt))
    if rc:
        raise MsspeError(rc, "msspe_group_rows: bad argument")
    rows = np.zeros(max(cnt.value, 1), dtype=np.uint32)
    rc = L.msspe_group_rows(n, n_members, member, rows.ctypes.data, int(rows.size), C.byref(cnt))
    if rc:
        raise MsspeError(rc, "msspe_group_rows failed")
    return rows[:cnt.value]


def rccl_available(library: str | None = None) -> tuple[bool, str]:
    """(loadable with every entry point the group uses, reason if not) -- msspe_group_rccl_available; host only."""
    why = C.create_string_buffer(512)
    ok = load_library().msspe_group_rccl_available(library.encode() if library else None, why, 512)
    return bool(ok), why.value.decode()


class Group:
    """Several devices of one node in one process (include/msspe_hip.h msspe_group_*): one context per listed
    device; a device listed more than once = members sharing a card (the rehearsal mode, transport device-copy)."""

    def __init__(self, devices, params_path: str | None = None, transport: str | None = None):
        self.L = load_library()
        self.ptr = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = self.L.msspe_group_create(arr, len(devices), params_path.encode() if params_path else None,
                                       transport.encode() if transport else None, C.byref(self.ptr))
        if rc:
            msg = self.L.msspe_group_last_error(self.ptr).decode() if self.ptr else "allocation failed"
            if self.ptr:
                self.L.msspe_group_destroy(self.ptr)
                self.ptr = C.c_void_p()
            raise MsspeError(rc, msg)

    def close(self):
        if getattr(self, "ptr", None):
            self.L.msspe_group_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise MsspeError(rc, self.L.msspe_group_last_error(self.ptr).decode())

    @property
    def size(self) -> int:
        return int(self.L.msspe_group_size(self.ptr))

    @property
    def transport(self) -> str:
        return self.L.msspe_group_transport(self.ptr).decode()

    @property
    def transport_reason(self) -> str:
        """Why the copies run where transport "auto" wanted RCCL ("" otherwise)."""
        return self.L.msspe_group_transport_reason(self.ptr).decode()

    def set_option(self, key: str, value) -> None:
        self._check(self.L.msspe_group_set_option(self.ptr, key.encode(), str(value).encode()))

    def cross_dimer(self, pool, chem: Chem | None = None, threshold: float = -9000.0, want_bitmap=True):
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        rc_ = np.zeros(n, dtype=np.uint32)
        bm = np.zeros((n, (n + 63) // 64), dtype=np.uint64) if want_bitmap else None
        self._check(self.L.msspe_cross_dimer_group(self.ptr, buf, n, k, C.byref(chem), C.c_float(threshold),
                                                   rc_.ctypes.data, bm.ctypes.data if want_bitmap else None))
        return {"row_conflicts": rc_, "bitmap": bm}

    def cross_dimer_edges(self, pool, chem: Chem | None = None, threshold: float = -9000.0, capacity: int = 1 << 20):
        buf, n, k = _ascii(pool)
        chem = chem or Chem.ntthal()
        edges = np.zeros(capacity, dtype=np.dtype([("a", np.uint32), ("b", np.uint32), ("dg", np.float32)]))
        count = C.c_uint64()
        rc = self.L.msspe_cross_dimer_edges_group(self.ptr, buf, n, k, C.byref(chem), C.c_float(threshold),
                                                  edges.ctypes.data, capacity, C.byref(count))
        if rc:
            err = MsspeError(rc, self.L.msspe_group_last_error(self.ptr).decode())
            err.count = int(count.value)
            raise err
        return edges[:count.value], int(count.value)

    def oligo_stats(self, pool, chem: Chem | None = None):
        buf, n, k = _ascii(pool)
        chem = chem or Chem.primer3()
        out = {name: np.empty(n) for name in ("tm", "gc", "self_any", "self_end", "hairpin")}
        self._check(self.L.msspe_oligo_stats_group(self.ptr, buf, n, k, C.byref(chem),
                                                   *[out[x].ctypes.data for x in out]))
        return out
