"""The third session campaign's generators and expected values without a GPU (tests/session_campaign3_model.py):
schedules are deterministic per seed and keep the rules of the module's docstring, the committed seeds together hold
every family, k, option, chain order, boundary size, weight mode, R value, entry form and optional output, and every
session's expected values are not vacuous.  Conditions on the generators, not measurements: a seed that fails one needs
another generator or another seed."""
import numpy as np
import pytest

import panel_thin_depth_model as dm
import session_campaign3_model as s3
from pair_bound_window_model import window_bound_pair, window_tables

N_CALLS = 27
ALTERNATING = ("matrix", "select", "slab")
MANY = ("thin_thal_depth", "select_depth", "thin_w", "select_w", "graph")      # two calls or more in every session


def test_eight_committed_seeds():
    assert len(s3.SEEDS) == 8 == len(set(s3.SEEDS)) and s3.N_CALLS == N_CALLS


@pytest.mark.parametrize("seed", s3.SEEDS)
def test_schedule_is_deterministic(seed):
    a, b = s3.schedule(seed), s3.schedule(seed)
    assert [c.describe() for c in a] == [c.describe() for c in b]
    for x, y in zip(a, b):
        if x.kind in ("decide_w", "window_plane"):
            assert x.data()["pool"] == y.data()["pool"]
        if x.kind in ("cover_rule", "tubes_rule"):
            assert x.data()["words"] == y.data()["words"]
        if x.kind in ("thin_w", "select_w", "thin_depth", "thin_thal_depth", "select_depth"):
            np.testing.assert_array_equal(x.data()["g"], y.data()["g"])
            assert x.data()["fwd"] == y.data()["fwd"] and x.data()["rev"] == y.data()["rev"]
            if "w" in x.data():
                np.testing.assert_array_equal(x.data()["w"], y.data()["w"])


def by_place(calls, name):
    return sorted((c for c in calls if c.block.startswith(name + ":")), key=lambda c: c.pos)


@pytest.mark.parametrize("seed", s3.SEEDS)
def test_schedule_rules(seed):
    calls = s3.schedule(seed)
    assert len(calls) == N_CALLS and [c.index for c in calls] == list(range(N_CALLS))
    # neighbours follow each other, forwards or reversed, and nothing else stands between them
    for name, chain in s3.CHAINS.items():
        mine = [c for c in calls if c.block.startswith(name + ":")]
        assert [c.index for c in mine] == list(range(mine[0].index, mine[0].index + len(chain))), name
        assert [c.kind for c in mine] == list(chain if mine[0].block.endswith("fwd") else chain[::-1]), name
    # rule 1: every new family with two calls: both ends of its range, another k where it has one
    for family in MANY:
        mine = [c for c in calls if c.kind == family]
        assert len(mine) >= 2 and {c.size for c in mine} == {"large", "small"}, family
        ks = {(c.p.get("k"), c.p.get("k_a")) for c in mine}
        assert len(ks) >= 2, family
    # the alternating chains: one window geometry, a strictly smaller matrix straight after a larger one and the reverse
    for name in ALTERNATING:
        mine = by_place(calls, name)
        assert len({(c.p["seg"], c.p["stride"], c.p["W"]) for c in mine if "seg" in c.p}) == 1
        sizes = [c.size for c in mine]
        twin = [i for i, c in enumerate(mine) if c.p.get("twin")]
        assert twin == ([3] if name == "select" else [])
        for i, (a, b) in enumerate(zip(sizes, sizes[1:])):
            assert (a == b) == (i + 1 in twin), (name, sizes)
        shapes = [s3.matrix_shape(c) for c in mine]
        steps = [(a, b) for a, b in zip(shapes, shapes[1:]) if a and b]
        assert any(b[0] < a[0] and b[1] < a[1] for a, b in steps), (name, shapes)
        assert any(b[0] > a[0] and b[1] > a[1] for a, b in steps), (name, shapes)
    # the matrix chain: weighted, plain, depth, weighted (other size, other weights), held depth, plain
    matrix = by_place(calls, "matrix")
    assert matrix[0].p["weights"] != matrix[3].p["weights"] and matrix[0].size != matrix[3].size
    assert matrix[2].p["R"] in (1, 2, 3) and matrix[4].p["R"] in (2, 3)
    # the select chain: R >= 2 at T = 3, then select and its twin at R = 1 on the very same inputs, then the _rule form
    select = by_place(calls, "select")
    assert select[1].p["R"] >= 2 and select[1].p["T"] == 3 and select[3].p["R"] == 1
    assert select[3].data() is select[2].data()
    assert {key: v for key, v in select[3].p.items() if key not in ("R", "twin")} == select[2].p
    assert select[4].p["form"] == "screen" and select[0].p["form"] in ("dev", "packed")
    # the graph chain: one chemistry and one pair of thresholds; the consumers screen another pool than their neighbours
    graph = by_place(calls, "graph")
    assert len({c.p["rule2"] for c in graph}) == 1 and graph[0].p["rule2"] in s3.GRAPH_RULES
    assert [c.p.get("variant") for c in graph] == ["bitmap", None, "edges", None, None, "ab"]
    assert graph[0].data() is not graph[1].data() and graph[1].data() is graph[2].data()
    assert graph[3].data() is graph[0].data() and graph[3].data() is not graph[2].data()
    assert graph[4].p["form"] == "screen" and None not in graph[4].p["screen_rule"]       # use_end = 1 beside use_any
    assert graph[5].p["k_a"] != graph[5].p["k_b"]
    # the slab chain: mode 2 for the tolerant seeding, a held rule for the weighted selection, and the slab that splits
    slab = by_place(calls, "slab")
    assert slab[3].p["mode"] == "end1" and slab[4].p["rule"] in ("any", "end1") and slab[1].p["mode"] in ("any", "end1")
    split = [c for c in calls if c.p.get("split")]
    assert len(split) == 1 and split[0] in (slab[1], slab[4]) and split[0].size == "large"
    assert split[0].option == ("site_list_cap_log2", 12)
    after = slab[slab.index(split[0]) + 1] if split[0] is slab[1] else slab[3]
    assert after.size == "small"                     # a pass whose list fits stands next to the split one
    # the bound chain: one pool; windowed screen, window plane, packed screen, the single-rule graph, windowed screen
    bound = by_place(calls, "bound")
    assert all(c.data() is bound[0].data() for c in bound)
    assert [c.p.get("window") for c in bound] == [1, None, 0, None, 1] and bound[3].p["variant"] == "any"
    assert len({(c.p["k"], c.p["chem"], c.p["thr"], c.p["n"]) for c in bound}) == 1
    for c in calls:
        p = c.p
        # rule 2: sizes
        if c.kind in ("decide_w", "decide", "window_plane") or p.get("variant") == "any":
            n = p["n"]
            assert n == len(c.data()["pool"]) and (n in (63, 64, 65) or (250 <= n <= 400 and n % 24)), n
        if c.kind == "window_plane":
            (r0, r1), (c0, c1) = p["rows"], p["cols"]
            assert 0 <= r0 < r1 <= p["n"] and 0 <= c0 < c1 <= p["n"] and (r1 - r0) * (c1 - c0) <= s3.PLANE_PAIRS
            assert (p["n"] <= 80) == ((r0, r1, c0, c1) == (0, p["n"], 0, p["n"])) and (p["n"] <= 80 or min(r0, c0) > 0)
        if c.kind in ("cover_rule", "tubes_rule") or p.get("variant") in ("bitmap", "edges"):
            n, words = p["n"], c.data()["words"]
            assert len(words) == n == len(set(words)) and (n in (63, 64, 65) or (150 <= n <= 300 and n % 24)), n
            assert p["k"] in s3.GRAPH_KS
        if p.get("variant") == "ab":
            assert max(p["n_a"], p["n_b"]) <= 110 and {p["k_a"], p["k_b"]} == {13, 20}
        if "seg" in p:
            g = c.data()["g"]
            assert 8 <= g.shape[0] <= 40 and 1200 <= g.shape[1] <= 5000 + p["stride"]
            assert (g.shape[1] - p["seg"]) % p["stride"], "a trailing partial segment"
            assert (g == ord("-")).any() and (g == ord("N")).any()
        if "n_f" in p:
            d = c.data()
            assert (len(d["fwd"]), len(d["rev"])) == (p["n_f"], p["n_r"]) and 10 <= min(p["n_f"], p["n_r"])
            assert max(p["n_f"], p["n_r"]) <= 130
        if c.kind in ("select", "select_depth", "select_w"):
            d = c.data()
            assert len(set(d["fwd"] + d["rev"])) == p["n_f"] + p["n_r"]       # a graph's nodes are distinct
        # rule 3: weights
        if c.kind in ("thin_w", "select_w"):
            w = c.data()["w"]
            assert w.shape == (s3.n_segments_of(c.data()["g"], p),) and w.min() >= 0 and int(w.sum()) <= s3.LIMIT
            if p["weights"] == "ones":
                assert (w == 1).all()
            else:
                assert (w == 0).any() and (w == 1).any() and ((w > 1) & (w < 10)).any() and 1 <= (w >= 10 ** 6).sum() <= 4
                assert (int(w.sum()) == s3.LIMIT) == (p["weights"] == "limit")
        # rule 4: depth panels carry shadows and a forced later duplicate
        if c.kind in ("thin_depth", "thin_thal_depth"):
            d = c.data()
            sh = dm.shadows(d["fwd"], d["rev"], d["forced"])
            last = p["n_f"] - 1
            assert sh.sum() >= 3 and d["forced"][last] and not sh[last] and sh[d["fwd"].index(d["fwd"][last])]
        # rule 5: options
        if c.option:
            name, value = c.option
            assert name in s3.options_of(c) and value != s3.option_default(name)
            if name == "conflict_graph_block_rows":
                assert 1 < value < p["rows_n"] and p["rows_n"] % value
            else:
                assert c.option in [x[:2] for x in s3.OPTIONS]


def test_committed_seeds_cover_every_item():
    have, large_first = set(), 0
    for seed in s3.SEEDS:
        calls = s3.schedule(seed)
        have |= s3.covered(calls)
        large_first += calls[0].size == "large"
    assert not s3.required() - have, sorted(s3.required() - have, key=repr)
    assert 0 < large_first < len(s3.SEEDS)           # sessions that grow first and sessions that shrink first


@pytest.fixture(scope="module")
def session_counters():
    """Every expected value of every committed session, once: counters per seed (and the calls, for the cross-checks)."""
    out = {}
    for seed in s3.SEEDS:
        calls = s3.schedule(seed)
        for c in calls:
            s3.expect(c)
        out[seed] = (s3.counters(calls), calls)
    return out


@pytest.mark.parametrize("seed", s3.SEEDS)
def test_expected_values_are_not_vacuous(session_counters, seed):
    n, _calls = session_counters[seed]
    assert n["graph_all_three_kinds"]
    assert n["edge_list_truncated"]
    assert n["depth_keeps_more_and_has_shadows"]
    assert n["weights_change_the_picks"]
    assert n["zero_weight_segment_covered"]
    assert n["select_depth_layer_2"]
    assert n["slab_splits"]
    assert n["decide_some_conflicts"]
    assert n["window_culls"]


def test_weights_and_depths_across_the_sessions(session_counters):
    """Rules 3 and 4 on the expected values: a total of exactly 2^32 - 1, all ones with the unweighted call's outputs,
    segments with fewer than R representatives, R = 1 with select's bytes, every optional output asked for once."""
    totals, ones, thin, twins, asked = set(), 0, set(), 0, set()
    for seed, (_n, calls) in session_counters.items():
        for c in calls:
            want = s3.expect(c)
            if c.kind in ("thin_w", "select_w"):
                totals.add(c.stats["total"])
                if c.p["weights"] == "ones":
                    ones += 1
                    for key in [key for key in want if key.startswith("twin.")]:
                        assert s3.same(want[key], want[key[5:]]), (c.describe(), key)
                    assert any(key.startswith("twin.") for key in want)
            if c.kind in ("thin_depth", "thin_thal_depth"):
                if c.stats["thin_segments"] > 0:
                    thin.add(seed)
            if c.p.get("twin"):
                twins += 1
                flat = s3.expect(next(x for x in calls if x.block == c.block and x.kind == "select"))
                for key in ("order", "gains", "keep", "tube", "barred", "tubes_used", "rounds"):
                    assert s3.same(want[key], flat[key]), key
                assert s3.same(want["as select.covered"], flat["covered"])
            if c.kind == "graph" and c.p["variant"] in ("bitmap", "edges", "any"):
                asked |= {"rc", "kinds", "bitmap"} - {{1: "rc", 2: "kinds", 3: "bitmap"}.get(c.p["optional"])}
    assert s3.LIMIT in totals and ones >= 2 and thin == set(s3.SEEDS) and twins == 8 and asked == {"rc", "kinds", "bitmap"}


@pytest.mark.parametrize("seed", s3.SEEDS)
def test_the_window_plane_model_is_the_pair_model(session_counters, seed):
    """The numpy plane the window plane is compared with against pair_bound_window_model.window_bound_pair, the pair
    by pair form the family's own tests pin it to, on a sample of the session's block."""
    import msspe_amd as m
    _n, calls = session_counters[seed]
    c = next(c for c in calls if c.kind == "window_plane")
    want = s3.expect(c)
    pool, p = c.data()["pool"], c.p
    pk = window_tables(m, None, s3.chem_obj(m, p["chem"]), p["thr"])
    rows, cols = pool[p["rows"][0]:p["rows"][1]], pool[p["cols"][0]:p["cols"][1]]
    rng = np.random.default_rng(seed)
    for i, j in zip(rng.integers(0, len(rows), 40), rng.integers(0, len(cols), 40)):
        lb = window_bound_pair(pk, rows[i], cols[j])
        assert want["window.model"][i, j] == (np.inf if lb is None else lb), (rows[i], cols[j])
    assert c.stats["finite"] > 0
