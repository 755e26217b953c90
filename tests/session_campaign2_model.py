"""The second session campaign (tools/random_campaign_session.py --campaign 2, tests/test_gpu_session_campaign2.py): the
entry points added after the first campaign (tests/session_campaign_model.py) -- decision-only screens through the bound
chain, the three bound diagnostic planes, coverage and thinning scored with thal, excluding and tolerant stage A, the
selection by coverage -- chained with the older calls they share device state with, all on ONE msspe_ctx.

Expected values come from the CPU oracle (oracle/pyoracle.py) and the numpy models under tests/ alone, never from the
engine.  This module holds no GPU code and does not import torch; run_session() is handed the engine and the package by
its caller.  The bound planes' expected values read the product's host-only table builders (msspe_amd.capi
host_bound_tables / host_bound_packed, no device), imported where they are needed.

Chains of a session (CHAINS; neighbours run straight after each other, each chain forwards or reversed per seed):
    matrix     thin -> thin_thal -> select -> tolerant (mode 0) -> thin           (ctx->thin: incidence matrix, rounds)
    site       thal -> cov_thal -> thin_thal -> tolerant (mode 1 | 2) -> thal     (site_work, plane words, DP workspace,
                                                                                   overflow lists)
    graph      cover -> select (screens itself, T = 3) -> tubes -> select (caller's bitmap, T = 1) -> cover  (ctx->cover)
    chem       decide -> end -> cov_thal "any" -> tolerant mode 2 -> decide on another pool, same k
               (one chemistry and one numeric threshold: the three cut kinds of that chemistry side by side; the last
                call is the second one on a ChemEntry whose bound_share[k] is recorded.  The bound stage runs for cuts
                <= 0 only, so the threshold is negative; as a temperature it makes every match stable, and the held /
                not held split is the site chain's business)
    bound      decide square -> decide ab -> bound_plane -> any with planes -> decide square   (one pool; the last
               equals the first byte for byte)
and two excluding calls outside the chains: 27 calls, then the first three once more.

Rules (checked by tests/test_session_campaign2_model.py):
  * every new family with two calls or more is called at a large and at a small end of its range, with another k where
    it has one (the chem chain's two decide calls share k: bound_share is recorded per length);
  * inside the matrix and site chains the sizes alternate (one window geometry per chain), so a call whose padded
    primer count and segment-group count are both smaller directly follows a larger one, and a larger one a smaller one;
  * primer counts per direction include 63, 64 and 65 across the seeds; decide pools are at 63 / 64 / 65 or at 250..400
    with n % 24 != 0; alignments leave a partial trailing segment and hold '-' and 'N' runs;
  * every device output starts as 0xA5 with 64 guard elements behind its defined extent; row_conflicts starts at 5;
  * with probability 1/4 a call runs under one non-default option its family reads (OPTIONS), restored afterwards, on
    which no expected value depends (a draw on a family that reads none passes to the next call that does);
  * the first three calls are repeated at the end and return the same bytes;
  * all comparisons are exact: integers equal, doubles bit for bit."""
from __future__ import annotations

import time

import numpy as np

import coverage_thal_model as ctm
import panel_select_model as sm
import panel_thin_model as ptm
import panel_thin_thal_model as ttm
import pyoracle as o
import session_campaign_model as scm
from pair_bound_list_model import class_plane, skewed_pool
from pair_bound_model import mixed_pool
from pair_bound_packed_model import NONE, packed_tables, plane_model
from session_campaign_model import (GUARD, RC_BASE, Call, Device, alignment, bits, chem_args, chem_obj, differences,
                                    graph, guard_ok, image, pack_bits, rc, same, sentinel, tables, window_primers)
from stage_a_excluding_model import CachedSegments, ExcludingModel
from stage_a_seeded_model import SeededModel
from stage_a_tolerant_model import TolerantModel, seed_incidence

__all__ = ["same"]

# the seeds of the suite (tests/test_session_campaign2_model.py holds what they have to cover together)
SEEDS = (1, 2, 3, 4, 5, 15, 49, 123)

NEW_FAMILIES = ("decide", "bound_plane", "cov_thal", "thin_thal", "excluding", "tolerant", "select")
CHAINS = {
    "matrix": ("thin", "thin_thal", "select", "tolerant", "thin"),
    "site": ("thal", "cov_thal", "thin_thal", "tolerant", "thal"),
    "graph": ("cover", "select", "tubes", "select", "cover"),
    "chem": ("decide", "end", "cov_thal", "tolerant", "decide"),
    "bound": ("decide", "decide", "bound_plane", "any", "decide"),
}
KS = {
    "decide": (9, 12, 13), "cov_thal": (8, 13, 16, 24), "thin_thal": (8, 13, 16, 24), "tolerant": (8, 13, 16, 24),
    "select": (13, 16, 20), "excluding": (5, 8, 13, 16), "thin": scm.KS["thin"], "thal": scm.KS["bg_thal"],
    "end": scm.KS["end"],
}
WINDOWS = scm.WINDOWS
# (name, value for the call, default) and per family the options an entry point of it reads (csrc/capi.cpp)
OPTIONS = (("pair_bound", 1, "auto"), ("pair_bound", 0, "auto"), ("pair_mirror", 0, "auto"),
           ("pair_bound_list", 0, "auto"), ("pair_bound_packed", 0, "auto"), ("pair_bound_packed", 1, "auto"),
           ("list_cap_log2", 20, 0), ("site_list_cap_log2", 12, 22), ("thin_thal_unique", 0, 1), ("stage_a_graph", 0, 1))
_PAIR = ("pair_bound", "pair_mirror", "pair_bound_list", "pair_bound_packed", "list_cap_log2")
OPTIONS_OF = {
    "decide": _PAIR, "any": _PAIR, "cov_thal": ("site_list_cap_log2",), "thal": ("site_list_cap_log2",),
    "thin_thal": ("site_list_cap_log2", "thin_thal_unique"), "excluding": ("stage_a_graph",),
    "tolerant": ("stage_a_graph", "site_list_cap_log2", "thin_thal_unique"),
}
CHEM_THRESHOLDS = (-9000.0, -6000.0, -3000.0)     # the chem chain's one number: a dG cut the bound stage runs at
# thresholds at which matches of k bases within two mismatches fall on both sides (test_gpu_coverage_thal.py: 30 / 40 at 13)
TM_OF_K = {8: (4.0, 10.0), 13: (30.0, 40.0), 16: (40.0, 48.0), 20: (50.0, 56.0), 24: (56.0, 62.0)}
PLANE_PAIRS = 6500                                # pairs of a bound_plane block (the models take seconds per 10,000)


class Call2(Call):
    def data(self):
        if self._data is None:
            self._data = DATA[self.kind](self)
        return self._data


# ---- the schedule -----------------------------------------------------------------------------------------------------

def schedule(seed: int) -> list[Call2]:
    """The calls of a session, without the replay of the first three.  Deterministic per seed."""
    rng = np.random.default_rng([seed, 0x5E5520])
    first_large = bool(rng.integers(0, 2))
    X, Y = ("large", "small") if first_large else ("small", "large")
    blocks = []
    for name, chain in CHAINS.items():
        fwd = bool(rng.integers(0, 2))
        items = [(kind, pos) for pos, kind in enumerate(chain)]
        blocks.append((f"{name}:{'fwd' if fwd else 'rev'}", items if fwd else items[::-1]))
    blocks += [("single", [("excluding", 0)]), ("single", [("excluding", 1)])]
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    # sizes by chain position: the matrix and site chains alternate; thin_thal stands at an even place of one and an odd
    # place of the other, and the chem and graph chains give cov_thal, tolerant, select and decide their other end
    sizes = {"matrix": (X, Y, X, Y, X), "site": (X, Y, X, Y, X), "chem": (X, Y, X, X, Y), "graph": (X, Y, Y, X, Y),
             "bound": (Y,) * 5}
    calls, n_single = [], 0
    for name, items in blocks:
        for kind, pos in items:
            chain = name.split(":")[0]
            if chain == "single":
                size = (X, Y)[n_single]
                n_single += 1
            else:
                size = sizes[chain][pos]
            c = Call2(seed, len(calls), kind, kind, size, name)
            c.pos = pos
            calls.append(c)
    chains = {}
    for c in calls:
        c.shared = {}                                  # what the old families cache per call (scored sites)
        c.chain = chains.setdefault(c.block if c.block != "single" else f"single{c.index}", {})
    ks = {f: [KS[f][i] for i in rng.permutation(len(KS[f]))] for f in KS}
    geoms = {name: WINDOWS[int(rng.integers(0, 3))] for name in chains}
    chem_pick = (("ntthal", "primer3")[int(rng.integers(0, 2))],
                 float(CHEM_THRESHOLDS[int(rng.integers(0, len(CHEM_THRESHOLDS)))]))
    drawn = {}
    for c in calls:
        r = c.rng(1)
        chain = c.block.split(":")[0]
        c.geom = geoms[c.block if c.block != "single" else f"single{c.index}"]
        if c.kind in KS:
            if c.kind == "decide" and "k" in c.chain:
                c.p["k"] = c.chain["k"]                # one pool (bound), one bound_share record (chem)
            else:
                c.p["k"] = ks[c.kind].pop(0) if ks[c.kind] else KS[c.kind][int(r.integers(0, len(KS[c.kind])))]
                if c.kind == "decide":
                    c.chain["k"] = c.p["k"]
        if chain == "chem":
            c.p["chem"], c.p["thr"] = chem_pick
        PARAMS[c.kind](c, r)
        drawn[c.index] = bool(r.random() < 0.25)
    carry = 0
    for c in calls:
        names = OPTIONS_OF.get(c.kind)
        if not names:
            carry += drawn[c.index]
            continue
        if drawn[c.index] or carry:
            carry -= not drawn[c.index]
            r = c.rng(5)
            mine = [x for x in OPTIONS if x[0] in names]
            c.option = mine[int(r.integers(0, len(mine)))][:2]
    return calls


def option_default(name):
    return next(x[2] for x in OPTIONS if x[0] == name)


# ---- parameters and inputs of every kind of call -----------------------------------------------------------------------

def p_align2(c, r):
    """scm.p_align at the chain's window geometry."""
    seg, stride, W = c.geom
    if c.size == "large":
        rows, length = int(r.integers(24, 41)), int(r.integers(3000, 5001))
    else:
        rows, length = int(r.integers(8, 13)), int(r.integers(1200, 2001))
    if seg == 60:                                  # 30-column strides: many segments per row
        rows, length = max(8, rows // 2), max(1200, length // 2)
    c.p.update(rows=rows, length=length, seg=seg, stride=stride, W=W)


def p_panel(c, r):
    """Primers per direction: 66..130 at the large end -- one direction at 63, 64 or 65 every other time -- and 10..31 at
    the small end, so that a large panel's padded count (>= 192) is above a small one's (64)."""
    if c.size == "large":
        n = [int(r.integers(66, 131)), int(r.integers(66, 131))]
        if r.integers(0, 2):
            n[int(r.integers(0, 2))] = int(r.choice([63, 64, 65]))
    else:
        n = [int(r.integers(10, 32)), int(r.integers(10, 32))]
    k = c.p["k"]
    c.p.update(n_f=n[0], n_r=n[1], M=int(r.integers(0, 2 if k <= 8 else 3)), E=int(r.choice([0, 1, 3])))


def p_scored(c, r):
    """chemistry, thal mode and temperature of a thal-scored call (the chem chain brings its own)."""
    c.p.setdefault("chem", ("ntthal", "primer3")[int(r.integers(0, 2))])
    c.p.setdefault("thr", float(TM_OF_K[c.p["k"]][int(r.integers(0, 2))]))
    c.p["mode"] = "any" if c.block.startswith("chem:") else ("any", "end1")[int(r.integers(0, 2))]


def p_thin2(c, r):
    p_align2(c, r)
    p_panel(c, r)
    c.p.update(M=int(r.integers(0, 4)), E=int(r.choice([0, 1, 3, c.p["k"]])), min_gain=int(r.integers(1, 3)),
               n_forced=int(r.integers(0, 4)), form=("host", "dev", "packed")[int(r.integers(0, 3))])


def p_cov_thal(c, r):
    p_align2(c, r)
    p_panel(c, r)
    p_scored(c, r)
    if c.kind == "cov_thal":                       # exact matches alone all hold at these temperatures
        c.p["M"] = max(1, c.p["M"])
    c.p["form"] = ("host", "dev", "packed")[int(r.integers(0, 3))]


def p_thin_thal(c, r):
    p_cov_thal(c, r)
    c.p.update(min_gain=int(r.integers(1, 3)), n_forced=int(r.integers(0, 4)))


def p_select(c, r):
    p_align2(c, r)
    p_panel(c, r)
    chain = c.block.split(":")[0]
    if chain == "graph":                           # the screen-derived graph at T = 3, then a caller's bitmap at T = 1
        screen = c.pos == 1
        T = 3 if screen else 1
    else:
        screen, T = bool(r.integers(0, 4) == 0), int(r.choice([1, 3]))
    c.p.update(form="screen" if screen else ("bitmap", "dev", "packed")[int(r.integers(0, 3))], T=T,
               min_gain=int(r.integers(1, 3)), n_forced=int(r.integers(0, 4)), skewed=bool(r.integers(0, 2)),
               rule=(0, 0, "any", "end1")[int(r.integers(0, 4))])
    if c.p["rule"]:
        p_scored(c, r)
        c.p["mode"] = c.p["rule"]
    if screen:
        c.p.update(screen_chem="ntthal", screen_thr=float(r.choice([-6000.0, -9000.0])))


def p_tolerant(c, r):
    p_align2(c, r)
    chain = c.block.split(":")[0]
    k = c.p["k"]
    c.p.update(iters=int(r.integers(12, 41)), mms=int(r.integers(1, 3)),
               n_seed=int(r.integers(70, 131)) if c.size == "large" else int(r.integers(5, 32)),
               M=int(r.integers(1, 2 if k <= 8 else 3)), E=int(r.choice([0, 1, 3])),
               form=("host", "packed", "both")[int(r.integers(0, 3))], n_exclude=int(r.integers(0, 3)))
    if chain == "matrix":
        c.p["mode"] = 0
    else:
        p_scored(c, r)
        c.p["mode"] = "end1" if chain == "chem" else ("any", "end1")[int(r.integers(0, 2))]


def p_excluding(c, r):
    p_align2(c, r)
    c.p.update(iters=int(r.integers(12, 41)), mms=int(r.integers(1, 3)),
               form=("host", "packed", "both")[int(r.integers(0, 3))])


def p_decide(c, r):
    chain = c.block.split(":")[0]
    if chain == "bound" and "n" in c.chain:
        c.p.update({key: c.chain[key] for key in ("n", "pool", "pseed", "chem", "thr")})
    else:
        if c.size == "large":
            n = int(r.integers(250, 401))
            n += n % 24 == 0
        else:
            n = int(r.choice([63, 64, 65]))
        k = c.p["k"]
        c.p.update(n=n, pool=("skewed", "mixed")[int(r.integers(0, 2))], pseed=int(r.integers(1 << 30)))
        c.p.setdefault("chem", ("ntthal", "primer3", "ntthal37")[int(r.integers(0, 3))])
        c.p.setdefault("thr", float(r.choice([-2500.0, -5000.0] if k <= 9 else [-9000.0, -5000.0, -2500.0])))
        if chain == "bound":
            c.chain.update({key: c.p[key] for key in ("n", "pool", "pseed", "chem", "thr")})
    n = c.p["n"]
    if chain == "bound":
        c.p["form"] = {0: "square", 1: "ab", 4: "square"}[c.pos]
    else:
        c.p["form"] = ("square", "dev", "ab")[int(r.integers(0, 3))]
    if c.p["form"] == "dev":
        r0 = int(r.integers(0, n)); r1 = int(r.integers(r0 + 1, n + 1))
        c0 = int(r.integers(0, n)); c1 = int(r.integers(c0 + 1, n + 1))
        c.p["rect"] = (r0, r1, c0, c1)
    if c.p["form"] == "ab":
        c.p["n_a"] = int(r.integers(1, n))


def p_bound_plane(c, r):
    p_decide_shared(c)
    n = c.p["n"]
    if n * n <= PLANE_PAIRS:
        rows, cols = (0, n), (0, n)
    else:                                          # a block off the origin, more than one wave of columns
        nr, nc = int(r.integers(30, 49)), int(r.integers(66, 131))
        r0, c0 = int(r.integers(0, n - nr + 1)), int(r.integers(0, n - nc + 1))
        rows, cols = (r0, r0 + nr), (c0, c0 + nc)
    c.p.update(rows=rows, cols=cols)


def p_decide_shared(c):
    """The bound chain's pool, for the calls of it that are not decide (their place in the chain is never the first)."""
    if "n" not in c.chain:                         # a reversed chain starts with decide as well: this is not reached
        raise AssertionError("the bound chain starts and ends with decide")
    c.p.update({key: c.chain[key] for key in ("k", "n", "pool", "pseed", "chem", "thr")})


def p_any_planes(c, r):
    p_decide_shared(c)
    n = c.p["n"]
    r0 = int(r.integers(0, n)); r1 = int(r.integers(r0 + 1, n + 1))
    c0 = int(r.integers(0, n)); c1 = int(r.integers(c0 + 1, n + 1))
    c.p.update(planes=True, dev=("planes", "edges")[int(r.integers(0, 2))], rect=(r0, r1, c0, c1))


def p_tubes(c, r):
    c.p.update(T=int(r.choice([3, 64])), T2=int(r.choice([1, 3, 64])))
    scm.p_graph(c, r)


PARAMS = {"thin": p_thin2, "thin_thal": p_thin_thal, "cov_thal": p_cov_thal, "select": p_select, "tolerant": p_tolerant,
          "excluding": p_excluding, "decide": p_decide, "bound_plane": p_bound_plane, "any": p_any_planes,
          "thal": scm.p_bg, "end": scm.p_end, "cover": scm.p_graph, "tubes": p_tubes}


def d_align2(c):
    r = c.rng(2)
    return {"g": alignment(r, c.p["rows"], c.p["length"], c.p["seg"], c.p["stride"])}


def distinct_primers(r, g, n_f, n_r, p):
    """n_f forward and n_r reverse primers off the alignment's windows, no word twice (a graph's nodes are distinct)."""
    k = p["k"]
    out = ([], [])
    have = set()
    for _ in range(20):
        fwd, rev = window_primers(r, g, max(n_f, n_r) + 8, k, p["seg"], p["stride"], p["W"])
        for d, words in ((0, fwd), (1, rev)):
            for w in words:
                if w not in have and len(out[d]) < (n_f, n_r)[d]:
                    have.add(w)
                    out[d].append(w)
        if len(out[0]) == n_f and len(out[1]) == n_r:
            return out
    raise AssertionError("no distinct primer set")


def d_panel(c):
    d = d_align2(c)
    d["fwd"], d["rev"] = distinct_primers(c.rng(3), d["g"], c.p["n_f"], c.p["n_r"], c.p)
    if "n_forced" in c.p:
        r, n = c.rng(4), c.p["n_f"] + c.p["n_r"]
        forced = np.zeros(n, dtype=np.uint8)
        forced[r.choice(n, size=c.p["n_forced"], replace=False)] = 1
        d["forced"] = forced if c.p["n_forced"] else None
    return d


def d_select(c):
    d = d_panel(c)
    d["b"] = graph(c.rng(5), c.p["n_f"] + c.p["n_r"], c.p["skewed"])
    return d


def d_tolerant(c):
    d = d_align2(c)
    r, p = c.rng(3), c.p
    fwd, rev = window_primers(r, d["g"], p["n_seed"], p["k"], p["seg"], p["stride"], p["W"])
    d["seeds"] = [list(dict.fromkeys(fwd)), list(dict.fromkeys(rev))]
    return d


def decide_pool(p):
    """skewed_pool / mixed_pool of p["n"] oligos with reverse-complement partners (conflicts at every threshold drawn)."""
    n, k = p["n"], p["k"]
    pool = skewed_pool(k, n - 23, p["pseed"]) if p["pool"] == "skewed" else mixed_pool(k, n - 7, p["pseed"])
    assert len(pool) == n
    n_random = n - (23 if p["pool"] == "skewed" else 7)
    for j in range(min(8, n_random // 4)):
        pool[n_random // 2 + j] = rc(pool[j])
    return pool


def d_decide(c):
    key = ("pooldata", c.p["pseed"], c.p["n"])
    if key not in c.chain:
        c.chain[key] = {"pool": decide_pool(c.p)}
    return c.chain[key]


DATA = {"thin": scm.d_thin, "thin_thal": d_panel, "cov_thal": d_panel, "select": d_select, "tolerant": d_tolerant,
        "excluding": d_align2, "decide": d_decide, "bound_plane": d_decide, "any": d_decide, "thal": scm.d_bg,
        "end": scm.d_end, "cover": scm.d_graph, "tubes": scm.d_graph}


# ---- what the rules of the matrix and site chains look at ------------------------------------------------------------

def group_size(W: int, k: int) -> int:
    """Segments per matrix word (csrc/coverage_mm.hip MismatchCoverage::group_size: 2,048 positions a round, 64 at most)."""
    return max(1, min(64, 2048 // (W - k + 1)))


def matrix_shape(c):
    """(primers or seeds padded to 64, segment groups) of a call that fills an incidence matrix; None for the others."""
    if c.kind not in ("thin", "thin_thal", "cov_thal", "select", "tolerant"):
        return None
    p, g = c.p, c.data()["g"]
    n = max(len(s) for s in c.data()["seeds"]) if c.kind == "tolerant" else p["n_f"] + p["n_r"]
    n_seg = g.shape[0] * ptm.n_partitions(g.shape[1], p["seg"], p["stride"])
    S = group_size(p["W"], p["k"])
    return (n + 63) // 64 * 64, -(-n_seg // S)


# ---- expected values ---------------------------------------------------------------------------------------------------

def u64(x) -> np.ndarray:
    """float64 as its bits: what "bit for bit" compares."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def scored_result(c):
    """coverage_thal_model.coverage_thal of a call's alignment and panel under its rule."""
    d, p = c.data(), c.p
    return ctm.coverage_thal(tables(), d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], p["M"], p["E"],
                             p["mode"], p["thr"], chem_args(p["chem"]))


def e_cov_thal(c):
    res = scored_result(c)
    recs = res["matches"]
    c.stats = {"matches": len(recs), "stable": int((recs["stable"] != 0).sum())}
    want = {"held": res["held"], "t_best": u64(res["t_best"]), "primer_segments": res["primer_segments"],
            "primer_held": res["primer_held"], "count": res["count"]}
    for f in ("primer", "segment", "offset", "mismatches", "stable"):
        want[f"matches.{f}"] = np.ascontiguousarray(recs[f])
    for f in ("dg", "t"):
        want[f"matches.{f}"] = u64(recs[f])
    return want


def thin_want(c, greedy):
    keep, order, gains, covered, c_all, c_kept, _rounds = greedy
    c.stats = {"kept": int(keep.sum()), "dropped": int((keep == 0).sum())}
    return {"keep": keep, "order": order, "gains": gains,
            "covered": np.asarray(covered).astype(np.uint8).reshape(c.data()["g"].shape[0], -1), "covered_all": c_all,
            "covered_kept": c_kept}


def e_thin_thal(c):
    H = ttm.held_incidence(scored_result(c))
    return thin_want(c, ptm.greedy(H, c.p["min_gain"], c.data()["forced"]))


def select_graph(c):
    d, p = c.data(), c.p
    if p["form"] != "screen":
        return d["b"]
    _, _, cf, _ = o.pool_pairs(tables(), d["fwd"] + d["rev"], chem_args(p["screen_chem"]), p["screen_thr"], want_dg=False)
    return cf.astype(bool)


def e_select(c):
    d, p = c.data(), c.p
    if p["rule"]:
        I = ttm.held_incidence(scored_result(c))
    else:
        I = ptm.incidence(d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], p["M"], p["E"])
    B = select_graph(c)
    res = sm.select(I, B, p["T"], p["min_gain"], d["forced"])
    sm.check_independent(res, B, d["forced"])
    free = sm.select(I, np.zeros_like(B), p["T"], p["min_gain"], d["forced"])
    c.stats = {"picks": len(res["order"]), "barred": int(res["barred"].sum()), "edges": int(B.sum()),
               "graph_matters": res["order"].tolist() != free["order"].tolist()}
    c.graph = B
    want = {key: res[key] for key in ("order", "gains", "keep", "tube", "barred", "covered_all", "covered_kept",
                                      "tubes_used", "rounds")}
    want["covered"] = res["covered"].astype(np.uint8).reshape(d["g"].shape[0], -1)
    return want


def segments_of(c):
    d, p = c.data(), c.p
    seqs = [bytes(row).decode() for row in d["g"]]
    return CachedSegments(o.Segments(seqs, p["seg"], p["stride"], p["W"], p["k"]))


def e_tolerant(c):
    d, p = c.data(), c.p
    segs = segments_of(c)
    fields = (p["seg"], p["stride"], p["W"], p["k"])
    want, differs, covered = {}, False, 0
    d["exclude"] = {}
    for direction in (0, 1):
        plain = SeededModel(segs, direction)
        won = [w for w, _ in plain.candidates(p["iters"], p["mms"])]
        exclude = won[1:1 + p["n_exclude"]]
        d["exclude"][direction] = exclude or None
        model = TolerantModel(segs, direction, d["g"], fields, exclude)
        kw = dict(tables=tables(), args=chem_args(p["chem"])) if p["mode"] else {}
        got, cov, parts = model.candidates_tolerant(p["iters"], p["mms"], d["seeds"][direction], p["M"], p["E"],
                                                    p["mode"], p.get("thr", 0.0), **kw)
        want[f"d{direction}.words"] = [w for w, _ in got]
        want[f"d{direction}.freqs"] = np.array([f for _, f in got], dtype=np.uint32)
        want[f"d{direction}.covered"], want[f"d{direction}.parts"] = cov, parts
        _, exact = seed_incidence(d["g"], fields, direction, d["seeds"][direction], 0, 0)
        differs |= not np.array_equal(exact.any(axis=0).reshape(cov.shape), cov != 0)
        covered += int(cov.sum())
    c.stats = {"covered": covered, "differs_from_exact": bool(differs)}
    return want


def e_excluding(c):
    d, p = c.data(), c.p
    segs = segments_of(c)
    want, removed = {}, 0
    d["lists"] = {}
    for direction in (0, 1):
        plain = SeededModel(segs, direction)
        won = plain.candidates(p["iters"], p["mms"])
        want[f"plain{direction}.words"] = [w for w, _ in won]
        want[f"plain{direction}.freqs"] = np.array([f for _, f in won], dtype=np.uint32)
        r = c.rng(10 + direction)
        w = [x for x, _ in won]
        vocab = plain.vocab
        quarter = [vocab[i] for i in r.choice(len(vocab), max(1, len(vocab) // 4), replace=False) if vocab[i] not in w[1:3]]
        exclude = w[:1] + w[3:5] + quarter + quarter[:5] + ["ACGTTGCAAGCTTGCA"[:p["k"]]]
        seed = w[1:3]
        d["lists"][direction] = (seed, exclude)
        got = ExcludingModel(segs, direction, exclude).candidates(p["iters"], p["mms"], seed=seed)
        want[f"sets{direction}.words"] = [x for x, _ in got]
        want[f"sets{direction}.freqs"] = np.array([f for _, f in got], dtype=np.uint32)
        removed += len(set(w) & set(exclude) - {x for x, _ in got})
    c.stats = {"removed": removed}
    return want


def oracle_pool(c):
    """The oracle's (dG, conflicts, t) of a decide pool: once per pool, shared by the chain's calls."""
    d, p = c.data(), c.p
    if "oracle" not in d:
        _, dg, cf, tt = o.pool_pairs(tables(), d["pool"], chem_args(p["chem"]), p["thr"], want_t=True)
        d["oracle"] = (dg, cf, tt)
    return d["oracle"]


def e_decide(c):
    p = c.p
    _, cf, _ = oracle_pool(c)
    c.stats = {"conflicts": int(cf.sum()), "pairs": cf.size}
    if p["form"] == "square":
        return {"bits": cf, "rc": cf.sum(1).astype(np.uint32)}
    if p["form"] == "ab":
        sub = cf[:p["n_a"], p["n_a"]:]
        return {"bits": sub, "rc": sub.sum(1).astype(np.uint32)}
    r0, r1, c0, c1 = p["rect"]
    sub = cf[r0:r1, c0:c1]
    rcw = np.full(p["n"], RC_BASE, dtype=np.uint32)
    rcw[r0:r1] += sub.sum(1).astype(np.uint32)
    return {"dev.bitmap": pack_bits(sub), "dev.rc": rcw}


def e_any_planes(c):
    p = c.p
    dg, cf, tt = oracle_pool(c)
    c.stats = {"conflicts": int(cf.sum()), "pairs": cf.size}
    return scm.square_want(dg, tt, cf, p["rect"], p["dev"], p["planes"], dg, scm.edge_dg)


def plane_values(bt, pick, unit_of):
    return np.where(pick == NONE, np.inf, unit_of(pick + bt["init"]))


def e_bound_plane(c):
    """The list plane in full (pair_bound_list_model's classes say where it is -inf and +inf, pair_bound_model's integer
    what it is elsewhere), and the exact-unit and packed values wherever the first stage bounds a pair itself."""
    import msspe_amd as m
    d, p = c.data(), c.p
    chem = chem_obj(m, p["chem"])
    rows, cols = d["pool"][p["rows"][0]:p["rows"][1]], d["pool"][p["cols"][0]:p["cols"][1]]
    ur, ri = np.unique(np.array(rows), return_inverse=True)
    uc, ci = np.unique(np.array(cols), return_inverse=True)
    bt = m.capi.host_bound_tables(None, chem, p["thr"])
    assert bt["usable"] == 1
    pick, _, _ = plane_model(bt, list(ur), list(uc))
    exact = plane_values(bt, pick, lambda x: x / bt["unit_inv"])[np.ix_(ri, ci)]
    cls = class_plane(rows, cols)
    lst = np.where((cls == "sym") | (cls == "over"), -np.inf, exact)
    assert (exact[cls == "none"] == np.inf).all() and np.isin(cls[exact == np.inf], ("none", "sym")).all()
    want = {"list": u64(lst), "exact.model": exact}
    pk = packed_tables(m, None, chem, p["thr"])
    want["packed.usable"] = int(pk["usable"])
    if pk["usable"]:
        pick, vmin, vmax = plane_model(pk, list(ur), list(uc))
        assert vmin == NONE or (pk["lo"] <= vmin and vmax <= pk["hi"])
        want["packed.model"] = plane_values(pk, pick, lambda x: x * pk["unit"])[np.ix_(ri, ci)]
    cut = m.g_cut(p["thr"])
    fin = np.isfinite(lst)
    c.stats = {"culled": int((lst[fin] > cut).sum()), "handed_on": int((lst[fin] <= cut).sum()) + int((lst == -np.inf).sum()),
               "classes": {x: int((cls == x).sum()) for x in ("row", "u", "over", "sym", "none")}}
    return want


EXPECT = {"thin": scm.e_thin, "thin_thal": e_thin_thal, "cov_thal": e_cov_thal, "select": e_select,
          "tolerant": e_tolerant, "excluding": e_excluding, "decide": e_decide, "bound_plane": e_bound_plane,
          "any": e_any_planes, "thal": scm.e_thal, "end": scm.e_end, "cover": scm.e_cover, "tubes": scm.e_tubes}
MODEL_ONLY = ("exact.model", "packed.model", "packed.usable")     # what a runner reads of `want` itself


def expect(c: Call) -> dict:
    """The expected outputs of a call (computed once), and c.stats: what the non-triviality counters read."""
    if c._want is None:
        c.stats = {}
        c._want = EXPECT[c.kind](c)
    return c._want


def counters(calls) -> dict:
    """What keeps a session from being vacuous, from the expected values of its calls (expect() has run on each)."""
    of = lambda kind: [c.stats for c in calls if c.kind == kind]
    return {
        "decide_some_conflicts": any(0 < s["conflicts"] < s["pairs"] for s in of("decide")),
        "bound_culls_and_hands_on": any(s["culled"] >= 1 and s["handed_on"] >= 1 for s in of("bound_plane")),
        "cov_thal_held_and_not": any(0 < s["stable"] < s["matches"] for s in of("cov_thal")),
        "thin_thal_drops_and_keeps": any(s["dropped"] >= 1 and s["kept"] >= 1 for s in of("thin_thal")),
        "select_graph_matters": any(s["graph_matters"] for s in of("select")),
        "tolerant_differs_from_exact": any(s["differs_from_exact"] for s in of("tolerant")),
        "excluding_removes_a_winner": any(s["removed"] >= 1 for s in of("excluding")),
    }


# ---- running a call on an engine --------------------------------------------------------------------------------------

def kmer_opt(m, p, iters=0, mms=0):
    return m.KmerOpt(p["seg"], p["stride"], p["W"], p["k"], iters, mms)


def r_cov_thal(c, eng, m, dv, want):
    p, d = c.p, c.data()
    res = eng.segment_coverage_thal(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"], chem_obj(m, p["chem"]),
                                    p["mode"], p["thr"], matches=True, packed=p["form"])
    got = {"held": res["held"], "t_best": u64(res["t_best"]), "primer_segments": res["primer_segments"],
           "primer_held": res["primer_held"], "count": res["count"]}
    for f in ("primer", "segment", "offset", "mismatches", "stable"):
        got[f"matches.{f}"] = np.ascontiguousarray(res["matches"][f])
    for f in ("dg", "t"):
        got[f"matches.{f}"] = u64(res["matches"][f])
    return got, []


def r_thin_thal(c, eng, m, dv, want):
    p, d = c.p, c.data()
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin_thal(
        d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"], chem_obj(m, p["chem"]), p["mode"], p["thr"],
        p["min_gain"], d["forced"], p["form"])
    return {"keep": keep, "order": order, "gains": gains, "covered": covered, "covered_all": c_all,
            "covered_kept": c_kept}, []


def r_select(c, eng, m, dv, want):
    p, d = c.p, c.data()
    rule = m.seed_rule(p["M"], p["E"], p["rule"], chem_obj(m, p["chem"]), p["thr"]) if p["rule"] else \
        m.seed_rule(p["M"], p["E"])
    if p["form"] == "screen":
        res = eng.panel_select(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], rule, None, p["T"], p["min_gain"], False,
                               d["forced"], "screen", chem=chem_obj(m, p["screen_chem"]), threshold=p["screen_thr"])
    else:
        res = eng.panel_select(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], rule, sm.pack_bitmap(d["b"]), p["T"],
                               p["min_gain"], False, d["forced"], p["form"])
    got = dict(res)
    got["rounds"] = eng.info("panel_select_rounds")
    problems = []
    try:                                            # the guarantees on the device's own result
        sm.check_independent(res, c.graph, d["forced"])
    except AssertionError as e:
        problems.append(f"the device's result breaks a guarantee of the selection: {e!r}")
    return got, problems


def r_tolerant(c, eng, m, dv, want):
    p, d = c.p, c.data()
    g = d["g"]
    opt = kmer_opt(m, p, p["iters"], p["mms"])
    rule = m.seed_rule(p["M"], p["E"], p["mode"], chem_obj(m, p["chem"]), p["thr"]) if p["mode"] else \
        m.seed_rule(p["M"], p["E"])
    seeds, excl = d["seeds"], d["exclude"]
    if p["form"] == "host":
        res = [eng.kmer_candidates_tolerant(g, opt, q, seeds[q], rule, exclude=excl[q]) for q in (0, 1)]
    else:
        handle = eng.put_rows_packed(g)
        try:
            if p["form"] == "packed":
                res = [eng.kmer_candidates_tolerant_packed(handle, g.shape[0], g.shape[1], opt, q, seeds[q], rule,
                                                           exclude=excl[q]) for q in (0, 1)]
            else:
                res = eng.kmer_candidates_tolerant_both_packed(handle, g.shape[0], g.shape[1], opt, seeds[0], seeds[1],
                                                               rule, exclude_fwd=excl[0], exclude_rev=excl[1])
        finally:
            eng.device_free(handle)
    got = {}
    for q in (0, 1):
        got[f"d{q}.words"], got[f"d{q}.freqs"], got[f"d{q}.covered"], got[f"d{q}.parts"] = res[q]
    return got, []


def r_excluding(c, eng, m, dv, want):
    p, d = c.p, c.data()
    g = d["g"]
    opt = kmer_opt(m, p, p["iters"], p["mms"])
    got = {}
    for q in (0, 1):
        got[f"plain{q}.words"], got[f"plain{q}.freqs"] = eng.kmer_candidates(g, opt, q)
    (s0, x0), (s1, x1) = d["lists"][0], d["lists"][1]
    if p["form"] == "host":
        res = [eng.kmer_candidates(g, opt, 0, seed=s0, exclude=x0), eng.kmer_candidates(g, opt, 1, seed=s1, exclude=x1)]
    else:
        handle = eng.put_rows_packed(g)
        try:
            if p["form"] == "packed":
                res = [eng.kmer_candidates_packed(handle, g.shape[0], g.shape[1], opt, 0, seed=s0, exclude=x0),
                       eng.kmer_candidates_packed(handle, g.shape[0], g.shape[1], opt, 1, seed=s1, exclude=x1)]
            else:
                res = eng.kmer_candidates_both_packed(handle, g.shape[0], g.shape[1], opt, seed_fwd=s0, seed_rev=s1,
                                                      exclude_fwd=x0, exclude_rev=x1)
        finally:
            eng.device_free(handle)
    for q in (0, 1):
        got[f"sets{q}.words"], got[f"sets{q}.freqs"] = res[q]
    return got, []


def r_decide(c, eng, m, dv, want):
    p, d = c.p, c.data()
    chem, pool, n = chem_obj(m, p["chem"]), d["pool"], p["n"]
    if p["form"] == "square":
        eng.pair_stage_stats()
        out = eng.cross_dimer(pool, chem, p["thr"], want_dg=False)
        c.mirrored = eng.pair_stage_stats()["bound_mirrored"]      # > 0: the bound first stage took the screen
        return {"bits": bits(out["bitmap"], n), "rc": out["row_conflicts"]}, []
    if p["form"] == "ab":
        n_a = p["n_a"]
        out = eng.cross_dimer_ab(pool[:n_a], pool[n_a:], chem, p["thr"], want_dg=False)
        return {"bits": bits(out["bitmap"], n - n_a), "rc": out["row_conflicts"]}, []
    r0, r1, c0, c1 = p["rect"]
    R, words = r1 - r0, (c1 - c0 + 63) // 64
    problems = []
    d_pool = dv.put(m.pack_oligos(pool))
    d_rc = dv.put(np.full(n, RC_BASE, dtype=np.uint32))
    d_bm = dv.put(sentinel(R * words, np.uint64))
    eng.cross_dimer_dev(d_pool, n, p["k"], chem, p["thr"], (r0, r1), (c0, c1), d_rc, d_bm)
    bm = dv.get(d_bm, R * words + GUARD, np.uint64)
    guard_ok(bm, R * words, "bitmap", problems)
    return {"dev.bitmap": bm[:R * words].reshape(R, words), "dev.rc": dv.get(d_rc, n, np.uint32)}, problems


def r_any_planes(c, eng, m, dv, want):
    return scm.r_square(c, m, dv, eng.cross_dimer, eng.cross_dimer_edges, eng.cross_dimer_dev, eng.cross_dimer_edges_dev,
                        c.p["k"], want)


def check_bounded(b, model, what, problems):
    """A first-stage plane against the model's values (tests/test_gpu_pair_bound_values.py check_values): a finite value
    is the model's, +inf stands only where the model has no chain, and there the plane is +inf or -inf."""
    if np.isnan(b).any():
        problems.append(f"{what}: NaN in the plane")
    fin = np.isfinite(b)
    if not np.array_equal(b[fin], model[fin]):
        bad = np.flatnonzero(b[fin] != model[fin])
        problems.append(f"{what}: {bad.size} of {int(fin.sum())} bounded pairs differ from the model, first got "
                        f"{b[fin][bad[0]]!r} expected {model[fin][bad[0]]!r}")
    if not (model[b == np.inf] == np.inf).all():
        problems.append(f"{what}: +inf where the model has a chain")
    if np.isfinite(b[model == np.inf]).any():
        problems.append(f"{what}: a value where the model has no chain")


def r_bound_plane(c, eng, m, dv, want):
    p, d = c.p, c.data()
    chem, pool, n = chem_obj(m, p["chem"]), d["pool"], p["n"]
    rows, cols = p["rows"], p["cols"]
    R, Cc = rows[1] - rows[0], cols[1] - cols[0]
    problems, planes = [], {}
    d_pool = dv.put(m.pack_oligos(pool))
    calls = [("exact", eng.cross_dimer_bound_dev), ("list", eng.cross_dimer_bound_list_dev)]
    if want["packed.usable"]:
        calls.insert(1, ("packed", eng.cross_dimer_bound_packed_dev))
    for name, call in calls:
        d_b = dv.put(sentinel(R * Cc, np.float64))
        call(d_pool, n, p["k"], chem, p["thr"], rows, cols, d_b)
        b = dv.get(d_b, R * Cc + GUARD, np.float64)
        guard_ok(b, R * Cc, f"{name} plane", problems)
        planes[name] = b[:R * Cc].reshape(R, Cc).copy()
    check_bounded(planes["exact"], want["exact.model"], "exact-unit plane", problems)
    kept = planes["exact"] != -np.inf             # what the first stage bounded itself the list stage leaves alone
    if not np.array_equal(u64(planes["list"][kept]), u64(planes["exact"][kept])):
        problems.append("list plane: a pair the first stage bounded has another value")
    if "packed" in planes:
        check_bounded(planes["packed"], want["packed.model"], "packed plane", problems)
        for v in (-np.inf, np.inf):                 # the sizing rules are shared
            if not np.array_equal(planes["packed"] == v, planes["exact"] == v):
                problems.append(f"packed plane: {v} at other pairs than in the exact-unit plane")
    got = {name: u64(b) for name, b in planes.items()}
    return got, problems


RUN = {"thin": scm.r_thin, "thin_thal": r_thin_thal, "cov_thal": r_cov_thal, "select": r_select,
       "tolerant": r_tolerant, "excluding": r_excluding, "decide": r_decide, "bound_plane": r_bound_plane,
       "any": r_any_planes, "thal": scm.r_thal, "end": scm.r_end, "cover": scm.r_cover, "tubes": scm.r_tubes}


def run_call(c: Call, eng, m, want) -> tuple[dict, list]:
    """One call on the engine, under its option if it has one (restored whatever happens): (outputs, problems)."""
    dv = Device(eng)
    try:
        if c.option:
            eng.set_option(*c.option)
        return RUN[c.kind](c, eng, m, dv, want)
    finally:
        try:
            if c.option:
                eng.set_option(c.option[0], option_default(c.option[0]))
        finally:
            dv.close()


def run_session(seed: int, eng, m, only: int | None = None, log=print) -> list[str]:
    """A whole session on one engine: every call against its expected value, the sentinels, the bound chain's last
    screen against its first, and the replay of the first three calls.  only: run the schedule up to and including that
    call and check that call alone.  Returns the failures, each naming seed, call index, kind, parameters and option."""
    calls = schedule(seed)
    failures, first, squares = [], {}, {}
    last = len(calls) - 1 if only is None else only
    for c in calls[:last + 1]:
        t0 = time.perf_counter()
        want = expect(c)
        t1 = time.perf_counter()
        got, problems = run_call(c, eng, m, want)
        t2 = time.perf_counter()
        if c.index < 3:
            first[c.index] = image(got)
        checked = {key: v for key, v in want.items() if key not in MODEL_ONLY}
        bad = [] if only is not None and c.index != only else differences(got, checked) + problems
        if c.kind == "decide" and c.block.startswith("bound:") and c.p["form"] == "square" and not bad:
            if squares.setdefault(c.block, image(got)) != image(got):
                bad.append("the bound chain's last square screen differs from its first")
            # pair_bound = auto measures the bound stage's share on the first call of a chemistry, threshold and length
            # and reuses the record: without an option both screens of the pool go to the same first stage
            if not c.option and squares.setdefault((c.block, "stage"), c.mirrored > 0) != (c.mirrored > 0):
                bad.append("the bound chain's last square screen took another first stage than its first")
        log(f"{c.describe()} model {t1 - t0:.2f} s engine {t2 - t1:.2f} s {c.stats} {'ok' if not bad else bad}")
        failures += [f"{c.describe()}: {b}" for b in bad]
    if only is None:
        for c in calls[:3]:
            got, problems = run_call(c, eng, m, expect(c))
            same_bytes = image(got) == first[c.index]
            log(f"replay of call {c.index} ({c.kind}) {'identical' if same_bytes else 'DIFFERS'}")
            if not same_bytes:
                failures.append(f"{c.describe()}: replay at the end of the session differs from the first run")
            failures += [f"{c.describe()} (replay): {b}" for b in problems]
    return failures


def models_only(seed: int, log=print) -> tuple[dict, float]:
    """Every schedule entry's expected value without an engine: (counters, model seconds)."""
    calls = schedule(seed)
    total = 0.0
    for c in calls:
        t0 = time.perf_counter()
        expect(c)
        dt = time.perf_counter() - t0
        total += dt
        log(f"{c.describe()} model {dt:.2f} s {c.stats}")
    return counters(calls), total


def covered(calls) -> set:
    """What a schedule exercises, as a set of items.  The committed seeds together have to hold every item of required()."""
    out = set()
    for c in calls:
        p = c.p
        out.add(("kind", c.kind, c.size) if c.kind in NEW_FAMILIES and c.kind != "bound_plane" else ("kind", c.kind))
        if c.kind in KS and c.kind in NEW_FAMILIES:
            out.add(("k", c.kind, p["k"]))
        if c.option:
            out.add(("option",) + tuple(c.option))
        if c.block != "single":
            out.add(("chain", c.block))
        if c.kind in ("tolerant", "excluding", "cov_thal", "thin_thal", "decide") or (c.kind == "select"
                                                                                      and c.block.startswith("matrix:")):
            out.add(("form", c.kind, p["form"]))
        if c.kind == "tolerant":
            out.add(("rule mode", {0: 0, "any": 1, "end1": 2}[p["mode"]]))
        if c.kind == "cov_thal":
            out.add(("cov_thal mode", p["mode"]))
        if c.kind == "select":
            out |= {("select graph", "screen" if p["form"] == "screen" else "bitmap"), ("T", p["T"]),
                    ("select incidence", "thal" if p["rule"] else "mismatch"), ("select forced", p["n_forced"] > 0)}
        if c.kind in ("thin", "thin_thal", "cov_thal", "select"):
            out |= {("primers", p["n_f"]), ("primers", p["n_r"])} & {("primers", x) for x in (63, 64, 65)}
        if c.kind == "decide":
            out.add(("decide n", p["n"] if p["n"] <= 65 else "large"))
            out.add(("decide pool", p["pool"]))
        if "seg" in p and c.kind in NEW_FAMILIES:
            out.add(("window", p["seg"]))
    return out


def required() -> set:
    out = {("kind", f, s) for f in NEW_FAMILIES if f != "bound_plane" for s in ("large", "small")}
    out |= {("kind", f) for f in ("bound_plane", "thin", "thal", "cover", "tubes", "end", "any")}
    out |= {("k", f, k) for f in NEW_FAMILIES if f in KS for k in KS[f]}
    out |= {("option",) + x[:2] for x in OPTIONS}
    out |= {("chain", f"{name}:{d}") for name in CHAINS for d in ("fwd", "rev")}
    out |= {("form", f, x) for f in ("tolerant", "excluding") for x in ("host", "packed", "both")}
    out |= {("form", f, x) for f in ("cov_thal", "thin_thal") for x in ("host", "dev", "packed")}
    out |= {("form", "decide", x) for x in ("square", "dev", "ab")}
    out |= {("form", "select", x) for x in ("bitmap", "dev", "packed")}
    out |= {("rule mode", x) for x in (0, 1, 2)} | {("cov_thal mode", x) for x in ("any", "end1")}
    out |= {("select graph", x) for x in ("screen", "bitmap")} | {("T", 1), ("T", 3)}
    out |= {("select incidence", x) for x in ("thal", "mismatch")} | {("select forced", True)}
    out |= {("primers", x) for x in (63, 64, 65)} | {("decide n", x) for x in (63, 64, 65, "large")}
    out |= {("decide pool", x) for x in ("skewed", "mixed")} | {("window", w[0]) for w in WINDOWS}
    return out
