"""The packed bound LIST stage without a GPU (option pair_bound_list_packed; csrc/thal_pairs_bound_list.hip
k_pairs_bound_list_packed).

The stage runs pair_bound_packed_model's recurrence -- the coarse tables of msspe_host_bound_packed, the packed first
stage's -- on the pairs of list U, whose tables hold 53..63 stored cells instead of at most 52.  What that needs, and
what is checked here on the 323-oligo skewed pool of the bound list stage's tests: (1) every value a cell of such a
pair publishes lies in the proven range [lo, hi], which does not depend on the number of stored cells (a left end term
plus at most 12 steps; a cell is at most its left end term), so that (2) value + bias never reaches bit 15 of the slot
word, whose coordinates start at bit 15 + 2; (3) the packed cull set, lbq > cutq, is a subset of the exact-unit cull
set, lb > cut: the coarser stage only hands more pairs to the exact chain."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from pair_bound_list_model import class_plane, skewed_pool
from pair_bound_packed_model import NONE, cells_and_pick, packed_tables, plane_model

THR = -9000.0
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def pool():
    p = skewed_pool(13, 300, seed=8113)
    assert len(p) == 323
    return p


@pytest.fixture(scope="module")
def tables(m):
    bt, pk = m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), packed_tables(m)
    assert bt["usable"] == 1 and pk["usable"] == 1
    bt["void"] = pk["void"]
    return bt, pk


@pytest.fixture(scope="module")
def u_pairs(pool):
    """(row, column) of every pair of class "u" (53..63 stored cells), and the distinct rows and columns they use."""
    at = np.argwhere(class_plane(pool, pool) == "u")
    assert len(at) > 10000
    return at


@pytest.fixture(scope="module")
def u_planes(pool, tables, u_pairs):
    """pick of the coarse and of the exact-unit model for every pair of the pool, and the extremes of the coarse cell values
    over all of them: computed once."""
    bt, pk = tables
    cls = class_plane(pool, pool)
    pq, vmin, vmax = plane_model(pk, pool, pool)
    px, _, _ = plane_model(bt, pool, pool)
    for a in (cls, pq, px):
        a.setflags(write=False)
    assert (cls == "u").sum() == len(u_pairs)
    return cls, pq, px, vmin, vmax


def test_cell_values_of_class_u_pairs_lie_in_the_proven_range(pool, tables, u_pairs):
    _, pk = tables
    rng = np.random.default_rng(1)
    lo, hi, n_cells = NONE, -NONE, 0
    for i, j in u_pairs[rng.choice(len(u_pairs), 300, replace=False)]:
        values, pick = cells_and_pick(pk, pool[i], pool[j])
        assert pick is not None and 53 <= len(values)      # (every cell, the last row's included)
        lo, hi, n_cells = min(lo, min(values)), max(hi, max(values)), max(n_cells, len(values))
    print(f"300 pairs of class u, up to {n_cells} cells: values {lo} .. {hi}, proven [{pk['lo']}, {pk['hi']}]")
    assert pk["lo"] <= lo and hi <= pk["hi"]


def test_field_never_reaches_bit_15(tables, u_planes):
    _, pk = tables
    cls, _, _, vmin, vmax = u_planes
    # (the extremes are over every cell of every pair of the pool, all of class u among them)
    assert pk["lo"] <= vmin and vmax <= pk["hi"]
    assert 0 <= vmin + pk["bias"] and vmax + pk["bias"] < (1 << 15)
    assert 0 <= pk["lo"] + pk["bias"] and pk["hi"] + pk["bias"] < (1 << 15)


def test_packed_cull_set_is_a_subset_of_the_exact_cull_set(tables, u_planes):
    bt, pk = tables
    cls, pq, px, _, _ = u_planes
    u = cls == "u"
    assert not (pq[u] == NONE).any() and not (px[u] == NONE).any()
    cull_q = u & (pq + pk["init"] > pk["cut"])
    cull_x = u & (px + bt["init"] > bt["cut"])
    print(f"{int(u.sum())} pairs of class u: {int(cull_q.sum())} culled in coarse units, {int(cull_x.sum())} in exact units")
    assert cull_q.sum() > 0 and not (cull_q & ~cull_x).any()
    # the coarse value, in exact units, is at most the exact one and less than 27 floored terms below it
    s = pk["shift"]
    dq, dx = (pq[u] + pk["init"]) << s, px[u] + bt["init"]
    assert (dq <= dx).all() and (dx - dq < 27 << s).all()


def test_kernel_resources(tmp_path):
    """The compiler's own remarks for the two kernels of thal_pairs_bound_list.hip, and the metadata of the device object
    it writes (tools/kernel_regs.sh): the packed instance fits 128 VGPRs without scratch, i.e. four waves per SIMD at
    1,024 threads; the exact-unit instance is what it was.  The compiler is build.sh's ($HIPCC, else ROCm's)."""
    csrc = ROOT / "open-msspe-design_amd" / "csrc"
    flags = re.search(r"FLAGS=\(([^)]*)\)", (ROOT / "open-msspe-design_amd" / "build.sh").read_text()).group(1).split()
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-x", "hip", "-c", "thal_pairs_bound_list.hip", "-o",
                          str(tmp_path / "bl.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True,
                         check=True).stderr
    kernels, name = {}, None
    for line in out.splitlines():
        if (f := re.search(r"Function Name: (\S+)", line)):
            name = f.group(1)
            kernels[name] = {}
        elif name and (f := re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)):
            kernels[name][f.group(1).strip()] = int(f.group(2))
    packed = [v for k, v in kernels.items() if "k_pairs_bound_list_packed" in k]
    exact = [v for k, v in kernels.items() if "k_pairs_bound_listE" in k]
    assert len(packed) == 1 and len(exact) == 1, list(kernels)
    print("packed:", packed[0], "exact:", exact[0])
    assert packed[0]["VGPRs"] <= 128 and packed[0]["AGPRs"] == 0 and packed[0]["ScratchSize"] == 0 and packed[0]["Occupancy"] == 4
    assert packed[0]["LDS Size"] <= 160 * 1024
    assert exact[0]["VGPRs"] == 248 and exact[0]["ScratchSize"] == 0 and exact[0]["Occupancy"] == 2
    # the device object's own record: 512 VGPRs per SIMD lane / 128 = four waves; nothing spilled to scratch
    notes = subprocess.run(["bash", str(ROOT / "tools" / "kernel_regs.sh"), str(tmp_path / "bl.o")], capture_output=True, text=True,
                           check=True).stdout
    rec = {ln.split()[0]: ln for ln in notes.splitlines() if "k_pairs_bound_list" in ln}
    got = [re.search(r"vgpr (\d+) \(spilled (\d+)\) sgpr \d+ \(spilled \d+\) lds (\d+) scratch (\d+)", ln).groups()
           for name, ln in rec.items() if "k_pairs_bound_list_packed" in name]
    assert len(got) == 1, notes
    vgpr, vspill, lds, scratch = map(int, got[0])
    assert vgpr <= 128 and 512 // vgpr == 4 and vspill == 0 and scratch == 0 and lds == packed[0]["LDS Size"]
