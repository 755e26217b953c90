"""od-msspe-hip --cover-on-device true: the cross-dimer screen and the vertex cover as one device call
(msspe_conflict_cover) give the CSV and the report of the default path (run_ntthal's edge list and the host
vertex_cover) byte for byte -- on three synthetic alignments at three thresholds, extending a panel, and with
--check-self-dimers false."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
HEADER = "direction,name,primers,gc,avg,std,tm\n"


@pytest.fixture(scope="module")
def alignments(tmp_path_factory):
    import msspe_amd
    out = []
    for c in range(3):
        g = np.concatenate([msspe_amd.synth.aligned_genomes(40, 12000, seed=310 + 3 * c + j) for j in range(3)])
        fa = tmp_path_factory.mktemp(f"cover{c}") / "in.fa"
        fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
        out.append(fa)
    return out


def run(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def same_both_ways(fa, tmp_path, *extra):
    base = run(fa, tmp_path / "host.csv", *extra)
    dev = run(fa, tmp_path / "dev.csv", "--cover-on-device", "true", *extra)
    assert dev[1] == base[1]
    assert dev[0] == base[0]
    return base


@pytest.mark.parametrize("c,thr", [(0, "-9000"), (1, "-6000"), (2, "-12000")])
def test_device_cover_gives_the_default_output(alignments, tmp_path, c, thr):
    _, csv = same_both_ways(alignments[c], tmp_path, "--delta-g-threshold", thr)
    assert csv.count(b"\n") > 1


def test_device_cover_with_a_panel(alignments, tmp_path):
    _, csv = run(alignments[0], tmp_path / "first.csv")
    rows = [line for line in csv.decode().splitlines()[1:] if line]
    panel = tmp_path / "panel.csv"
    panel.write_text(HEADER + "".join(r + "\n" for r in [r for r in rows if r.startswith("F,")][:4] +
                                      [r for r in rows if r.startswith("R,")][:3]))
    same_both_ways(alignments[0], tmp_path, "--existing-primers", str(panel))


def test_device_cover_without_self_dimer_checks(alignments, tmp_path):
    same_both_ways(alignments[1], tmp_path, "--check-self-dimers", "false", "--delta-g-threshold", "-7000")


def test_device_cover_and_devices_is_a_usage_error(alignments, tmp_path):
    r = subprocess.run([str(CLI), "-i", str(alignments[0]), "-o", str(tmp_path / "x.csv"), "--do-align", "false",
                        "--cover-on-device", "true", "--devices", "0,0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--cover-on-device" in (r.stderr + r.stdout)
