"""The seeded restatement of stage A (tests/stage_a_seeded_model.py) on the CPU: unseeded it is the oracle's greedy
loop; seeded with a prefix of the winners it continues where the unseeded loop was; seed order and duplicates do
not matter.  No GPU."""
import numpy as np
import pytest

from stage_a_seeded_model import SeededModel


def mutated(rows, length, rate, seed):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length)
    out = []
    for _ in range(rows):
        row = anc.copy()
        mut = rng.random(length) < rate
        row[mut] = rng.integers(0, 4, int(mut.sum()))
        out.append("".join("ACGT"[x] for x in row))
    return out


# (alignment, segment, stride, window, k, max_iterations, max_mismatch_segments); the k = 3 cases tie constantly
CASES = [
    ("synth", 500, 250, 50, 13, 1000, 1),
    ("ties", 40, 20, 12, 3, 1000, 1),
    ("ties", 40, 20, 12, 5, 9, 1),
    ("mut", 200, 100, 40, 9, 1000, 2),
    ("mut", 60, 30, 30, 8, 1000, 4),
]


def alignment(name):
    import msspe_amd
    if name == "synth":
        return [bytes(r).decode() for r in msspe_amd.synth.aligned_genomes(10, 3000)]
    if name == "ties":
        seqs = mutated(25, 400, 0.05, 5)
        return [s[:120] + "-" * 7 + s[127:300] + "N" * 3 + s[303:] for s in seqs]
    return mutated(30, 1500, 0.03, 9)


@pytest.fixture(scope="module")
def models(oracle):
    cache = {}

    def get(name, seg, stride, win, k, direction):
        key = (name, seg, stride, win, k)
        if key not in cache:
            cache[key] = oracle.Segments(alignment(name), seg, stride, win, k)
        segs = cache[key]
        return segs, SeededModel(segs, direction)
    return get


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-k{c[4]}-it{c[5]}-mm{c[6]}" for c in CASES])
def test_unseeded_model_equals_the_oracle(models, case, direction):
    name, seg, stride, win, k, iters, mm = case
    segs, model = models(name, seg, stride, win, k, direction)
    want = segs.candidates(direction, iters, mm)
    assert want, "the case selects nothing"
    assert model.candidates(iters, mm) == want
    assert model.candidates(iters, mm, seed=[]) == want


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("case", CASES[:4], ids=[f"{c[0]}-k{c[4]}" for c in CASES[:4]])
def test_prefix_invariant(models, case, direction):
    """Seeding with the first m winners and max_iterations - m returns exactly the remaining winners."""
    name, seg, stride, win, k, iters, mm = case
    _, model = models(name, seg, stride, win, k, direction)
    w = model.candidates(iters, mm)
    assert len(w) >= 3
    rng = np.random.default_rng(len(w))
    for m_ in sorted({1, 2, min(7, len(w) - 1), len(w) // 2, len(w) - 1}):
        seed = [x for x, _ in w[:m_]]
        rng.shuffle(seed)
        assert model.candidates(iters - m_, mm, seed=seed) == w[m_:], f"m = {m_}"


@pytest.mark.parametrize("direction", [0, 1])
def test_seed_order_and_duplicates_do_not_matter(models, direction):
    segs, model = models("ties", 40, 20, 12, 5, direction)
    present = sorted(model.index)
    rng = np.random.default_rng(3 + direction)
    seed = list(rng.choice(present, 12, replace=False)) + ["ACGTA" if "ACGTA" not in model.index else "TTTTT"]
    want = model.candidates(1000, 1, seed=seed)
    assert want != model.candidates(1000, 1)
    for trial in range(3):
        s = seed + seed[: 4 + trial]
        rng.shuffle(s)
        assert model.candidates(1000, 1, seed=s) == want
    # a seed absent from the index does nothing
    absent = [w for w in ("AAAAA", "CCCCC", "GGGGG", "TTTTT", "ACGTA") if w not in model.index]
    if absent:
        assert model.candidates(1000, 1, seed=absent) == model.candidates(1000, 1)
    # seeds are never winners
    assert not {x for x, _ in want} & set(seed)
