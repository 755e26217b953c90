"""Every msspe_conflict_graph* / *_rule entry point is declared in include/msspe_hip.h and exported by
libmsspe_hip.so, and the part that needs no device -- the checks made before a context is touched -- answers
MSSPE_ERR_ARG for a rule with both flags zero.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

NEW = ["msspe_conflict_graph_dev", "msspe_conflict_graph_ab_dev", "msspe_conflict_graph_edges_dev",
       "msspe_conflict_graph_ab_edges_dev", "msspe_conflict_graph", "msspe_conflict_graph_edges",
       "msspe_conflict_graph_ab_edges", "msspe_conflict_cover_rule", "msspe_conflict_tubes_rule",
       "msspe_panel_select_rule"]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def test_new_entry_points_are_declared_and_exported(m):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "msspe_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(msspe_[a-z0-9_]+)\s*\(", header))
    L = m.load_library()
    from msspe_amd.capi import EXPORTS
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in EXPORTS, name
    assert "msspe_conflict_rule" in header and "msspe_kind_edge" in header
    assert re.search(r"#define\s+MSSPE_KIND_ANY\s+1u", header) and re.search(r"#define\s+MSSPE_KIND_END\s+2u", header)


def test_rule_and_edge_layouts(m):
    from msspe_amd.capi import KIND_EDGE
    assert C.sizeof(m.ConflictRule) == 16 and KIND_EDGE.itemsize == 16
    r = m.ConflictRule.of(-12000.0, 25.0)
    assert (r.use_any, r.dg_threshold, r.use_end, r.end_tm_threshold) == (1, -12000.0, 1, 25.0)
    r = m.ConflictRule.of(None, 10.0)
    assert (r.use_any, r.use_end, r.end_tm_threshold) == (0, 1, 10.0)
    r = m.ConflictRule.of()
    assert (r.use_any, r.dg_threshold, r.use_end) == (1, -9000.0, 0)
    assert (m.KIND_ANY, m.KIND_END) == (1, 2)


def test_both_flags_zero_is_an_argument_error_without_a_device(m):
    """No context exists without a GPU; the entry points answer MSSPE_ERR_ARG (1) from their first checks."""
    L = m.load_library()
    chem = m.Chem.ntthal()
    none = m.ConflictRule(0, -9000.0, 0, 25.0)
    count = C.c_uint64(7)
    pool = b"ACGTACGTACGTA" * 2
    assert L.msspe_conflict_graph(None, pool, 2, 13, C.byref(chem), C.byref(none), None, None, None) == 1
    assert L.msspe_conflict_graph_edges(None, pool, 2, 13, C.byref(chem), C.byref(none), None, 0, C.byref(count)) == 1
    assert L.msspe_conflict_graph_ab_edges(None, pool, 2, 13, pool, 2, 13, C.byref(chem), C.byref(none), None, 0,
                                           C.byref(count)) == 1
    assert L.msspe_conflict_graph_dev(None, None, 2, 13, C.byref(chem), C.byref(none), 0, 2, 0, 2, None, None, None) == 1
    assert L.msspe_conflict_cover_rule(None, pool, 2, 13, C.byref(chem), C.byref(none), 0, None, None) == 1
    assert count.value == 7                       # nothing written
