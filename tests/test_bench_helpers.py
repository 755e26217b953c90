"""bench.py's host-side helpers that need no GPU: the stage-A roofline imported from the committed rocprofv3 summary
(bytes / SUM of kernel time per direction, labelled as imported)."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stage_a_roofline_comes_from_the_committed_kernel_stats():
    bench = load_bench()
    alg_bytes = 1190000 * (19.0 + 38 * 4.0 + 38 * 8.0 + 38 * 8.0 + 38 * 4.0)
    roof = bench.stage_a_kernel_roofline(alg_bytes)
    assert roof is not None, "profiles/r*_stage_a_kernel_stats.csv is tracked"
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and "imported" in roof["source"]
    # kernel time per direction: below the host wall time of the same workload, above the three sort passes alone
    assert 1.0 < roof["kernel_ms_per_direction"] < 20.0
    assert abs(roof["achieved"] - alg_bytes / (roof["kernel_ms_per_direction"] * 1e-3) / 1e9) < 1e-6
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9


def test_generated_scan_is_what_the_generator_writes():
    """open-msspe-design_amd/csrc/row_scan_pinned.inc (the row kernels' predecessor scan as inline asm) is generated:
    the committed file must be the generator's output, byte for byte."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_row_scan_asm.py")], capture_output=True, text=True, check=True)
    assert out.stdout == (ROOT / "open-msspe-design_amd" / "csrc" / "row_scan_pinned.inc").read_text()


def test_dump_outputs_writes_the_last_step_within_the_budget(tmp_path):
    """--dump-outputs: counts as float64, a fixed seeded sample of bitmap rows as float32 0/1 decisions (bit j of
    word w is column 64 w + j), under 64 MB, the same sample on every call; no bitmap, no sample files."""
    import numpy as np
    import torch
    bench = load_bench()
    n, r0 = 1000, 40
    rng = np.random.default_rng(3)
    words = rng.integers(-2**63, 2**63 - 1, size=(n - r0, (n + 63) // 64), dtype=np.int64)
    counts = rng.integers(0, n, size=n).astype(np.int32)
    for out in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(out), torch.from_numpy(counts), torch.from_numpy(words), n, r0)
    a = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(a) == ["bitmap_rows.npy", "bitmap_sample.npy", "row_conflicts.npy"]
    assert all(np.array_equal(a[k], np.load(tmp_path / "b" / k)) for k in a)
    assert a["row_conflicts.npy"].dtype == np.float64 and np.array_equal(a["row_conflicts.npy"], counts)
    rows, sample = a["bitmap_rows.npy"], a["bitmap_sample.npy"]
    assert rows.dtype == np.float64 and sample.dtype == np.float32 and sample.shape == (bench.DUMP_ROWS, n)
    assert np.all(np.diff(rows) > 0) and rows[0] >= r0 and rows[-1] < n
    col = np.arange(n)
    for i, r in enumerate(rows.astype(np.int64)):
        w = words[r - r0].view(np.uint64)
        assert np.array_equal(sample[i], (w[col // 64] >> (col % 64).astype(np.uint64)) & np.uint64(1))
    # a pool too wide for DUMP_ROWS rows: fewer rows, still under the budget
    wide = 1 << 20
    bench.dump_outputs(str(tmp_path / "c"), torch.zeros(wide, dtype=torch.int32),
                       torch.zeros((64, wide // 64), dtype=torch.int64), wide, 0)
    assert 0 < np.load(tmp_path / "c" / "bitmap_sample.npy").shape[0] < bench.DUMP_ROWS
    assert sum(p.stat().st_size for p in (tmp_path / "c").iterdir()) <= bench.DUMP_BYTES
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(counts), None, n, 0)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["row_conflicts.npy"]
