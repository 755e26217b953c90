"""The END screen's decision cut and the oracle identity it relies on (no GPU).

msspe_t_cut(thr) is the largest double x with round_fixed_f32(x, 2) < thr: the kernels flag a pair iff
t_end = max(0, t) > cut, which must be od-msspe's SELF_END rule ("%.2f" text parsed as f32, then <) applied to a pair.
END2(a, b) is END1(b, a) in the oracle, so one ordered-pair END1 screen answers both 3' ends."""
import numpy as np
import pytest

THRESHOLDS = [47.0, 10.0, 0.5, 0.005, 12.345, 12.335, 12.355, 46.995, 47.005, 0.0, -3.0]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_t_cut_is_the_exact_decision_boundary(m, oracle, thr):
    cut = m.t_cut(thr)
    thr32 = float(np.float32(thr))
    assert oracle.round_fixed_f32(cut, 2) < thr32
    assert not oracle.round_fixed_f32(float(np.nextafter(cut, np.inf)), 2) < thr32
    # the rule on values around the cut, and on t_end = 0 (no structure, or t <= 0)
    rng = np.random.default_rng(int(abs(thr) * 1000) + 7)
    for x in np.concatenate([cut + rng.normal(0, 0.01, 300), [0.0]]):
        assert (not oracle.round_fixed_f32(float(x), 2) < thr32) == (x > cut)


@pytest.mark.parametrize("thr", [0.0, -3.0])
def test_non_positive_thresholds_flag_every_pair(m, thr):
    assert 0.0 > m.t_cut(thr)     # t_end >= 0 always exceeds the cut


def _rand(rng, k):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, k))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_end2_is_end1_with_the_oligos_swapped(oracle, oracle_tables):
    rng = np.random.default_rng(2026)
    pairs = []
    for q in range(200):
        ka, kb = (int(x) for x in rng.integers(2, 33, 2))
        a, b = _rand(rng, ka), _rand(rng, kb)
        if q % 4 == 1 and ka % 2 == 0:          # self-complementary oligo 1
            a = a[: ka // 2] + _rc(a[: ka // 2])
        if q % 4 == 2 and kb % 2 == 0:          # self-complementary oligo 2
            b = b[: kb // 2] + _rc(b[: kb // 2])
        if q % 4 == 3:                          # b pairs with a's 3' end
            tail = a[-min(ka, kb):]
            b = _rc(tail) + b[len(tail):]
        pairs.append((a, b))
    structures = 0
    for a, b in pairs:
        e2 = oracle.thal(oracle_tables, a, b, oracle.END2)
        e1 = oracle.thal(oracle_tables, b, a, oracle.END1)
        assert e2.no_structure == e1.no_structure, (a, b)
        for f in ("dS", "dH", "dG", "t"):
            assert getattr(e2, f) == getattr(e1, f), (a, b, f)
        structures += not e1.no_structure
    assert structures > 100
