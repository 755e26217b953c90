"""The excluding restatement of stage A (tests/stage_a_excluding_model.py) on the CPU: without exclusions it is the
oracle's greedy loop and the seeded model; excluded words never win, and other words replace them; excluding the
whole vocabulary selects nothing.  The lists are the ones tests/test_gpu_stage_a_excluding.py runs on the device,
the one longer than the kernel's LDS budget among them.  No GPU."""
import pytest

from stage_a_excluding_model import CachedSegments, ExcludingModel, cases, exclusion_lists
from stage_a_seeded_model import SeededModel


@pytest.fixture(scope="module")
def built(oracle):
    import msspe_amd
    out = {}
    for name, rows, fields in cases(msspe_amd):
        raw = oracle.Segments([bytes(x).decode() for x in rows], *fields[:4])
        out[name] = (raw, CachedSegments(raw), fields)
    return out


NAMES = ["synth", "ties-k3", "ties-k5", "wide-k17"]


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_without_exclusions_it_is_the_oracle_and_the_seeded_model(built, name, direction):
    raw, segs, fields = built[name]
    want = raw.candidates(direction, fields[4], fields[5])
    assert len(want) >= 5, "the case selects too little"
    assert ExcludingModel(segs, direction).candidates(fields[4], fields[5]) == want
    assert ExcludingModel(segs, direction, []).candidates(fields[4], fields[5], seed=[]) == want
    seed = [w for w, _ in want[:2]]
    assert ExcludingModel(segs, direction).candidates(fields[4], fields[5], seed=seed) == \
        SeededModel(segs, direction).candidates(fields[4], fields[5], seed=seed)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_excluded_words_never_win_and_are_replaced(built, name, direction):
    _, segs, fields = built[name]
    plain = SeededModel(segs, direction)
    winners = plain.candidates(fields[4], fields[5])
    for label, (seed, exclude) in exclusion_lists(name, direction, plain.vocab, winners, fields[3]).items():
        model = ExcludingModel(segs, direction, exclude)
        got = model.candidates(fields[4], fields[5], seed=seed)
        assert not {w for w, _ in got} & set(exclude), label
        assert not set(model.index) & set(exclude), label
        # every other word keeps its own occurrences
        for w in list(model.index)[:50]:
            assert model.index[w] == plain.index[w], (label, w)
        if label == "d":
            assert got == [] and not model.index
        elif label == "c":
            assert not {w for w, _ in got} & set(seed)
            # the word in both lists is excluded: its seed does nothing
            assert got == ExcludingModel(segs, direction, exclude).candidates(fields[4], fields[5], seed=seed[1:])
        else:
            assert got != winners, label
            assert {w for w, _ in got} - {w for w, _ in winners}, f"{label}: no replacement word appeared"


@pytest.mark.parametrize("direction", [0, 1])
def test_order_and_duplicates_do_not_matter(built, direction):
    _, segs, fields = built["ties-k5"]
    plain = SeededModel(segs, direction)
    winners = plain.candidates(fields[4], fields[5])
    _, exclude = exclusion_lists("ties-k5", direction, plain.vocab, winners, 5)["b"]
    want = ExcludingModel(segs, direction, exclude).candidates(fields[4], fields[5])
    assert ExcludingModel(segs, direction, sorted(set(exclude), reverse=True)).candidates(fields[4], fields[5]) == want
    assert ExcludingModel(segs, direction, exclude + exclude[:9]).candidates(fields[4], fields[5]) == want
