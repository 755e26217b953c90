"""The second session campaign's generators and expected values without a GPU (tests/session_campaign2_model.py):
schedules are deterministic per seed and keep the rules of the module's docstring, the committed seeds together hold
every kind, k, option, rule mode, chain order, entry form, select form and tube limit, and every session's expected
values are not vacuous.  Conditions on the generators, not measurements: a seed that fails one needs another generator
or another seed."""
import numpy as np
import pytest

import session_campaign2_model as s2
from pair_bound_model import bound_pair

N_CALLS = 27


def test_eight_committed_seeds():
    assert len(s2.SEEDS) == 8 == len(set(s2.SEEDS))


@pytest.mark.parametrize("seed", s2.SEEDS)
def test_schedule_is_deterministic(seed):
    a, b = s2.schedule(seed), s2.schedule(seed)
    assert [c.describe() for c in a] == [c.describe() for c in b]
    for x, y in zip(a, b):
        if x.kind in ("decide", "end"):              # inputs held as lists of strings
            assert x.data()["pool"] == y.data()["pool"]
        if x.kind in ("select", "thin_thal", "tolerant"):
            np.testing.assert_array_equal(x.data()["g"], y.data()["g"])
            assert x.data().get("fwd") == y.data().get("fwd") and x.data().get("seeds") == y.data().get("seeds")


@pytest.mark.parametrize("seed", s2.SEEDS)
def test_schedule_rules(seed):
    calls = s2.schedule(seed)
    assert len(calls) == N_CALLS and [c.index for c in calls] == list(range(N_CALLS))
    # neighbours follow each other, forwards or reversed, and nothing else stands between them
    text = " ".join(c.kind for c in calls)
    for name, chain in s2.CHAINS.items():
        mine = [c for c in calls if c.block.startswith(name + ":")]
        assert [c.index for c in mine] == list(range(mine[0].index, mine[0].index + 5)), name
        kinds = [c.kind for c in mine]
        assert kinds == list(chain if mine[0].block.endswith("fwd") else chain[::-1]), name
        assert " ".join(kinds) in text
    assert sum(c.block == "single" for c in calls) == 2 == sum(c.kind == "excluding" for c in calls)
    # every new family with two calls: both ends of its range, another k
    for family in ("decide", "cov_thal", "thin_thal", "tolerant", "select", "excluding"):
        mine = [c for c in calls if c.kind == family]
        assert {c.size for c in mine} == {"large", "small"}, family
        assert len({c.p["k"] for c in mine}) >= 2, family
    # the matrix and site chains alternate: a strictly smaller matrix straight after a larger one, and the reverse
    for name in ("matrix", "site"):
        mine = [c for c in calls if c.block.startswith(name + ":")]
        assert [c.size for c in mine] in (["large", "small"] * 2 + ["large"], ["small", "large"] * 2 + ["small"])
        assert len({(c.p["seg"], c.p["stride"], c.p["W"]) for c in mine if "seg" in c.p}) == 1
        shapes = [s2.matrix_shape(c) for c in mine]
        steps = [(a, b) for a, b in zip(shapes, shapes[1:]) if a and b]
        assert any(b[0] < a[0] and b[1] < a[1] for a, b in steps), (name, shapes)
        assert any(b[0] > a[0] and b[1] > a[1] for a, b in steps), (name, shapes)
    matrix = [c for c in calls if c.block.startswith("matrix:")]
    assert next(c for c in matrix if c.kind == "tolerant").p["mode"] == 0
    site = [c for c in calls if c.block.startswith("site:")]
    assert next(c for c in site if c.kind == "tolerant").p["mode"] in ("any", "end1")
    # the graph chain: the screen-derived graph at T = 3 next to cover, the caller's bitmap at T = 1 next to the last cover
    graph = sorted((c for c in calls if c.block.startswith("graph:")), key=lambda c: c.pos)
    assert (graph[1].p["form"], graph[1].p["T"]) == ("screen", 3)
    assert graph[3].p["form"] in ("bitmap", "dev", "packed") and graph[3].p["T"] == 1
    # the chem chain: one chemistry, one number, the three cut kinds; both decide calls at one length, on two pools
    chem = sorted((c for c in calls if c.block.startswith("chem:")), key=lambda c: c.pos)
    assert len({(c.p["chem"], c.p["thr"]) for c in chem}) == 1 and chem[0].p["thr"] < 0.0
    assert chem[2].p["mode"] == "any" and chem[3].p["mode"] == "end1"      # kCutAnyT and kCutEndT beside kCutAnyDg
    assert chem[0].p["k"] == chem[4].p["k"] and chem[0].data()["pool"] != chem[4].data()["pool"]
    # the bound chain: one pool; square, ab, planes, any with planes, square
    bound = sorted((c for c in calls if c.block.startswith("bound:")), key=lambda c: c.pos)
    assert all(c.data() is bound[0].data() for c in bound)
    assert [c.p.get("form") for c in bound] == ["square", "ab", None, None, "square"] and bound[3].p["planes"]
    assert len({(c.p["k"], c.p["chem"], c.p["thr"], c.p["n"]) for c in bound}) == 1
    assert bound[0].p["k"] != chem[0].p["k"]
    # sizes
    for c in calls:
        if c.kind == "decide":
            n = c.p["n"]
            assert n == len(c.data()["pool"]) and (n in (63, 64, 65) or (250 <= n <= 400 and n % 24)), n
            assert c.p["k"] in (9, 12, 13)
        if c.kind == "bound_plane":
            (r0, r1), (c0, c1) = c.p["rows"], c.p["cols"]
            assert 0 <= r0 < r1 <= c.p["n"] and 0 <= c0 < c1 <= c.p["n"] and (r1 - r0) * (c1 - c0) <= s2.PLANE_PAIRS
            assert c1 - c0 > 64 or c.p["n"] <= 64      # more than one wave of columns wherever the pool has them
        if "seg" in c.p:
            g = c.data()["g"]
            assert 8 <= g.shape[0] <= 40 and 1200 <= g.shape[1] <= 5000 + c.p["stride"]
            assert (g.shape[1] - c.p["seg"]) % c.p["stride"], "a trailing partial segment"
            assert (g == ord("-")).any() and (g == ord("N")).any()
        if c.kind in ("thin_thal", "cov_thal", "select"):
            d = c.data()
            assert (len(d["fwd"]), len(d["rev"])) == (c.p["n_f"], c.p["n_r"]) and 10 <= min(c.p["n_f"], c.p["n_r"])
            assert max(c.p["n_f"], c.p["n_r"]) <= 130 and len(set(d["fwd"] + d["rev"])) == c.p["n_f"] + c.p["n_r"]
        if c.option:
            assert c.option in [x[:2] for x in s2.OPTIONS] and c.option[1] != s2.option_default(c.option[0])
            assert c.option[0] in s2.OPTIONS_OF[c.kind]


def test_committed_seeds_cover_every_item():
    have, large_first = set(), 0
    for seed in s2.SEEDS:
        calls = s2.schedule(seed)
        have |= s2.covered(calls)
        large_first += calls[0].size == "large"
    assert not s2.required() - have, sorted(s2.required() - have, key=repr)
    assert 0 < large_first < len(s2.SEEDS)           # sessions that grow first and sessions that shrink first


@pytest.fixture(scope="module")
def session_counters():
    """Every expected value of every committed session, once: counters per seed (and the calls, for the cross-checks)."""
    out = {}
    for seed in s2.SEEDS:
        calls = s2.schedule(seed)
        for c in calls:
            s2.expect(c)
        out[seed] = (s2.counters(calls), calls)
    return out


@pytest.mark.parametrize("seed", s2.SEEDS)
def test_expected_values_are_not_vacuous(session_counters, seed):
    n, _calls = session_counters[seed]
    assert n["decide_some_conflicts"]
    assert n["bound_culls_and_hands_on"]
    assert n["cov_thal_held_and_not"]
    assert n["thin_thal_drops_and_keeps"]
    assert n["select_graph_matters"]
    assert n["tolerant_differs_from_exact"]
    assert n["excluding_removes_a_winner"]


@pytest.mark.parametrize("seed", s2.SEEDS)
def test_the_plane_model_is_the_pair_model(session_counters, seed):
    """The numpy plane the bound planes are compared with against pair_bound_model.bound_pair, the model the family's
    own GPU tests use, on a sample of the session's block."""
    import msspe_amd as m
    _n, calls = session_counters[seed]
    c = next(c for c in calls if c.kind == "bound_plane")
    want = s2.expect(c)
    pool, p = c.data()["pool"], c.p
    bt = m.capi.host_bound_tables(None, s2.chem_obj(m, p["chem"]), p["thr"])
    rows, cols = pool[p["rows"][0]:p["rows"][1]], pool[p["cols"][0]:p["cols"][1]]
    rng = np.random.default_rng(seed)
    for i, j in zip(rng.integers(0, len(rows), 40), rng.integers(0, len(cols), 40)):
        lb = bound_pair(bt, rows[i], cols[j])
        assert want["exact.model"][i, j] == (np.inf if lb is None else lb), (rows[i], cols[j])
    assert c.stats["classes"]["row"] > 0 and np.isfinite(want["exact.model"]).any()
