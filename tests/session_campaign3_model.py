"""The third session campaign (tools/random_campaign_session.py --campaign 3, tests/test_gpu_session_campaign3.py): the
entry points added after the second campaign (tests/session_campaign2_model.py) -- thinning and selection to a coverage
depth, weighted coverage, the conflict graph under both rules and the rule forms of its consumers, the windowed bound
first stage, and the one slab loop of the thal-scored passes -- chained with the older calls whose device state they
share, all on ONE msspe_ctx.

Expected values come from the CPU oracle (oracle/pyoracle.py) and the numpy models under tests/ alone, never from the
engine.  This module holds no GPU code and does not import torch; run_session() is handed the engine and the package by
its caller.  The window plane's expected values read the product's host-only table builders (msspe_amd.capi
host_bound_packed / host_bound_window, no device), imported where they are needed.  Calls, generators, expected values
and runners of the chain partners are campaign I's and II's, imported as they are.

Chains of a session (CHAINS; neighbours run straight after each other, each chain forwards or reversed per seed):
    matrix   thin_w -> thin -> thin_depth (R 1..3) -> thin_w (other size, other weights) -> thin_thal_depth -> thin
             (ctx->thin: kInc, kCov, kGain, kLive beside kDepth, kMask and kWeight)
    select   select_w -> select_depth (R >= 2, T = 3) -> select -> select_depth at R = 1 on select's inputs ->
             select_w that screens itself under the rule      (ctx->select: kDepth, kPrimerMask, kWeight; ctx->cover;
             ctx->thin)
    graph    graph (bitmap, counts) -> cover_rule on another pool -> graph as ordered edges, capacity below the count
             -> tubes_rule -> select_depth that screens itself with use_end -> graph _ab, k_a != k_b
             (ctx->graph's per-rule planes, ctx->cover, one ChemEntry with kCutAnyDg and kCutEndT, two routes' lists)
    slab     background thal -> thin_thal_depth -> cov_thal -> tolerant mode 2 -> select_w under a held rule
             (site_work, the plane words, run_slabs; the large one of thin_thal_depth / select_w runs under
              site_list_cap_log2 12, so that every session splits a slab next to a pass whose list fits)
    bound    decide_w -> window_plane -> decide with pair_bound_window 0 -> graph with use_any only -> decide_w
             (one pool: list U and the packed tables; the single-rule graph is that screen; the last equals the first)
27 calls, then the first three once more.

Rules (checked by tests/test_session_campaign3_model.py):
  * every new family with two calls or more is called at a large and at a small end, with another k where it has one;
  * inside the matrix, select and slab chains the sizes alternate (one window geometry per chain); the one exception
    is select_depth at R = 1, which takes its neighbour select's inputs and has to return select's bytes;
  * primer counts per direction include 63, 64 and 65; a weighted or depth call leaves a last segment group of one
    segment; graph pools are at 63 / 64 / 65 and at 150..300 with n % 24 != 0; alignments leave a partial trailing
    segment and hold '-' and 'N' runs;
  * weights hold 0, 1, small values and a few large ones ("mixed"), the same with a total of exactly 2^32 - 1
    ("limit"), or all ones ("ones"): there the call also runs its unweighted form on the same inputs straight after
    the weighted one, and every shared output of the two has to be equal;
  * depth panels carry words listed twice (shadows), forced primers -- a forced later duplicate among them -- and
    segments with fewer than R representatives;
  * every device output starts as 0xA5 with 64 guard elements behind its defined extent; adding outputs start at a
    base; an edge list keeps the sentinel beyond min(count, capacity); an optional output is NULL in some draws;
  * with probability 1/4 a call runs under one non-default option its family reads (OPTIONS), restored afterwards, on
    which no expected value depends;
  * the first three calls are repeated at the end and return the same bytes;
  * all comparisons are exact: integers equal, doubles bit for bit; the window plane as its own GPU test compares it."""
from __future__ import annotations

import time

import numpy as np

import conflict_graph_model as cgm
import cover_round_model as crm
import panel_select_depth_model as sdm
import panel_select_model as sm
import panel_thin_depth_model as dm
import panel_thin_model as ptm
import panel_thin_thal_model as ttm
import panel_weighted_model as wm
import pyoracle as o
import session_campaign2_model as s2
import session_campaign_model as scm
from pair_bound_packed_model import NONE
from pair_bound_window_model import plane_model as window_plane_model, window_tables
from session_campaign_model import (GUARD, RC_BASE, Call, Device, bits, chem_args, chem_obj, differences, guard_ok, image,
                                    pack_bits, same, sentinel, tables)
from slab_split_model import slab_split_model

__all__ = ["same"]

# the seeds of the suite (tests/test_session_campaign3_model.py holds what they have to cover together)
SEEDS = (4, 6, 7, 49, 153, 159, 171, 388)

NEW_FAMILIES = ("thin_depth", "thin_thal_depth", "select_depth", "thin_w", "select_w", "graph", "cover_rule",
                "tubes_rule", "window_plane", "decide_w")
CHAINS = {
    "matrix": ("thin_w", "thin", "thin_depth", "thin_w", "thin_thal_depth", "thin"),
    "select": ("select_w", "select_depth", "select", "select_depth", "select_w"),
    "graph": ("graph", "cover_rule", "graph", "tubes_rule", "select_depth", "graph"),
    "slab": ("thal", "thin_thal_depth", "cov_thal", "tolerant", "select_w"),
    "bound": ("decide_w", "window_plane", "decide", "graph", "decide_w"),
}
N_CALLS = sum(len(c) for c in CHAINS.values())
# k of the families' own GPU tests (thal-scored ones: where s2.TM_OF_K has thresholds that split the matches)
KS = {
    "thin_depth": (13, 24), "thin_thal_depth": (13, 24), "select_depth": (13, 24), "thin_w": (13, 17, 24),
    "select_w": (13, 24), "decide_w": (9, 12, 13), "thin": scm.KS["thin"], "select": s2.KS["select"],
    "cov_thal": s2.KS["cov_thal"], "tolerant": s2.KS["tolerant"], "thal": scm.KS["bg_thal"],
}
GRAPH_KS = (13, 20)                                # the square pools'; _ab takes one of each
GRAPH_RULES = ((-9000.0, 10.0), (-12000.0, 25.0))  # (dG, END Tm) of tests/conflict_graph_model.py POOL_RULES
WINDOWS = scm.WINDOWS
# (name, value for the call, default); "rows": a value below the call's rows that does not divide them
OPTIONS = (("conflict_graph_block_rows", "rows", 0), ("site_list_cap_log2", 12, 22), ("thin_thal_unique", 0, 1),
           ("pair_bound_window", 0, "auto"), ("pair_bound_window", 1, "auto"), ("pair_bound_list", 0, "auto"),
           ("pair_bound_packed", 0, "auto"), ("list_cap_log2", 20, 0))
_PAIR = ("pair_bound_window", "pair_bound_list", "pair_bound_packed", "list_cap_log2")
_SITE = ("site_list_cap_log2", "thin_thal_unique")
# what an entry point of the family reads (csrc/capi.cpp); decide_w / decide set pair_bound_window themselves
OPTIONS_OF = {
    "graph": ("conflict_graph_block_rows",) + _PAIR, "cover_rule": ("conflict_graph_block_rows",) + _PAIR,
    "tubes_rule": ("conflict_graph_block_rows",) + _PAIR, "decide_w": _PAIR[1:], "decide": _PAIR[1:],
    "thal": ("site_list_cap_log2",), "cov_thal": ("site_list_cap_log2",), "thin_thal_depth": _SITE, "tolerant": _SITE,
}
WEIGHT_MODES = ("mixed", "limit", "ones")
LIMIT = wm.LIMIT
KIND_BASE = np.array([3, 4, 5], dtype=np.uint64)   # d_kind_counts is added to: the buffer starts at this
SPLIT_CAP = 1 << 12                                # the work list under site_list_cap_log2 12
PLANE_PAIRS = s2.PLANE_PAIRS


class Call3(Call):
    def data(self):
        if self._data is None:
            self._data = DATA[self.kind](self)
        return self._data


def chain_of(c) -> str:
    return c.block.split(":")[0]


# ---- the schedule -----------------------------------------------------------------------------------------------------

def schedule(seed: int) -> list[Call3]:
    """The calls of a session, without the replay of the first three.  Deterministic per seed."""
    rng = np.random.default_rng([seed, 0x5E5530])
    first_large = bool(rng.integers(0, 2))
    X, Y = ("large", "small") if first_large else ("small", "large")
    blocks = []
    for name, chain in CHAINS.items():
        fwd = bool(rng.integers(0, 2))
        items = [(kind, pos) for pos, kind in enumerate(chain)]
        blocks.append((f"{name}:{'fwd' if fwd else 'rev'}", items if fwd else items[::-1]))
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    # sizes by chain position.  matrix, select and slab alternate; select_depth at R = 1 (select, place 3) is select's
    # twin.  The families' second calls stand at the other end: thin_w X / Y, thin_thal_depth X (matrix) / Y (slab),
    # select_w Y / X (select) and X (slab), select_depth X / Y (select) and Y (graph), graph X / Y / X and Y (bound)
    sizes = {"matrix": (X, Y, X, Y, X, Y), "select": (Y, X, Y, Y, X), "slab": (X, Y, X, Y, X),
             "graph": (X, Y, Y, X, Y, X), "bound": (Y,) * 5}
    calls = []
    for name, items in blocks:
        for kind, pos in items:
            c = Call3(seed, len(calls), kind, kind, sizes[name.split(":")[0]][pos], name)
            c.pos = pos
            calls.append(c)
    chains = {}
    for c in calls:
        c.shared = {}                                  # what the old families cache per call (scored sites)
        c.chain = chains.setdefault(c.block, {})
    ks = {f: [KS[f][i] for i in rng.permutation(len(KS[f]))] for f in KS}
    geoms = {name: WINDOWS[int(rng.integers(0, 3))] for name in chains}
    rule_pick = GRAPH_RULES[int(rng.integers(0, 2))]
    modes = {f: [WEIGHT_MODES[i] for i in rng.permutation(3)] for f in ("thin_w", "select_w")}
    # the slab that splits: the large one of the slab chain's thin_thal_depth and select_w
    split_kind = "thin_thal_depth" if sizes["slab"][1] == "large" else "select_w"
    drawn = {}
    by_pos = sorted(calls, key=lambda c: (c.block, c.pos))   # parameters in chain order: a twin reads its neighbour's
    for c in by_pos:
        r = c.rng(1)
        chain = chain_of(c)
        c.geom = geoms[c.block]
        if c.kind in KS and not (chain == "select" and c.kind == "select_depth" and c.pos == 3):
            if c.kind in ("decide_w", "decide") and "k" in c.chain:
                c.p["k"] = c.chain["k"]                # one pool
            elif c.kind == "decide":
                raise AssertionError("decide stands behind decide_w")
            else:
                c.p["k"] = ks[c.kind].pop(0) if ks[c.kind] else KS[c.kind][int(r.integers(0, len(KS[c.kind])))]
                if c.kind == "decide_w":
                    c.chain["k"] = c.p["k"]
        if c.kind in modes:
            c.p["weights"] = modes[c.kind].pop(0)
        if chain == "graph":
            c.p["rule2"] = rule_pick
        if chain == "slab" and c.kind == split_kind:
            c.p["split"] = True
        PARAMS[c.kind](c, r)
        drawn[c.index] = bool(r.random() < 0.25)
    carry = 0
    for c in calls:
        names = options_of(c)
        if c.p.get("split"):                           # its option is set: a draw on it passes on
            c.option = ("site_list_cap_log2", 12)
            carry += drawn[c.index]
            continue
        if not names:
            carry += drawn[c.index]
            continue
        if drawn[c.index] or carry:
            carry -= not drawn[c.index]
            r = c.rng(5)
            mine = [x for x in OPTIONS if x[0] in names]
            name, value = mine[int(r.integers(0, len(mine)))][:2]
            c.option = (name, block_rows_below(c.p["rows_n"], r) if value == "rows" else value)
    return calls


def options_of(c):
    """The options a call's entry point reads; the selections read the graph's and the screens' only when they screen
    themselves, and the sites' only under a held rule."""
    if c.kind in ("select_depth", "select_w", "select"):
        names = ()
        if c.p["form"] == "screen":
            names += ("conflict_graph_block_rows",) + _PAIR
        if c.p.get("rule"):
            names += _SITE
        return names
    if c.kind == "graph" and c.p["variant"] == "ab":   # no square screen: the bound chain and the mirror do not run
        return ("conflict_graph_block_rows", "list_cap_log2")
    return OPTIONS_OF.get(c.kind, ())


def block_rows_below(rows: int, r) -> int:
    """A conflict_graph_block_rows below `rows` that does not divide them (rows >= 3)."""
    ok = [v for v in range(2, rows) if rows % v]
    return int(ok[int(r.integers(0, len(ok)))])


def option_default(name):
    return next(x[2] for x in OPTIONS if x[0] == name)


# ---- parameters and inputs of every kind of call -----------------------------------------------------------------------

def group_size(W: int, k: int) -> int:
    return s2.group_size(W, k)


def p_align3(c, r):
    """s2.p_align2; every third time the rows are moved inside their range so that the last segment group holds one
    segment (n_seg % S == 1), where the range has such a count."""
    s2.p_align2(c, r)
    if int(r.integers(0, 3)):
        return
    p = c.p
    S = group_size(p["W"], p["k"])
    lo, hi = (20, 40) if c.size == "large" else (8, 12)
    if p["seg"] == 60:
        lo, hi = max(8, lo // 2), max(8, hi // 2)
    P = ptm.n_partitions(p["length"], p["seg"], p["stride"])
    for rows in sorted(range(lo, hi + 1), key=lambda x: abs(x - p["rows"])):
        for dP in (0, 1, -1, 2, -2):
            length = p["length"] + dP * p["stride"]
            if S > 1 and 1200 <= length <= 5000 and (rows * (P + dP)) % S == 1:
                p.update(rows=rows, length=length)
                return


def p_thin3(c, r):
    """thin, thin_depth, thin_w: s2.p_thin2 at p_align3's shape."""
    s2.p_thin2(c, r)
    keep = dict(c.p)
    p_align3(c, c.rng(7))
    for key in ("rows", "length"):
        keep[key] = c.p[key]
    c.p.update(keep)
    if c.kind == "thin_depth":
        c.p["R"] = int(r.choice([1, 2, 2, 3, 3]))
        c.p["n_forced"] = max(1, c.p["n_forced"])
    if c.kind == "thin_w":                             # in weight units: 40 is above every small weight
        c.p["min_gain"] = int(r.choice([1, 2, 40] if c.p["weights"] != "ones" else [1, 2]))


def p_thin_thal_depth(c, r):
    s2.p_thin_thal(c, r)
    c.p.update(R=int(r.choice([2, 3])), n_forced=max(1, c.p["n_forced"]))
    p_split(c)


def p_split(c):
    """The slab chain's call that has to split a slab under site_list_cap_log2 12: the top of the large end's ranges,
    so that the matches its first slab lists pass 4,096 (tests/test_session_campaign3_model.py checks that they do)."""
    p = c.p
    if p.get("split"):
        p.update(rows=28 if p["seg"] == 60 else 40, n_f=max(p["n_f"], 124), n_r=max(p["n_r"], 124), M=2, E=0)


def p_sel3(c, r):
    """select, select_depth, select_w.  select_depth at R = 1 (select chain, place 3) takes select's parameters and
    inputs; the graph chain's select_depth and the select chain's last select_w screen their panel themselves."""
    chain = chain_of(c)
    if chain == "select" and c.pos == 3:
        c.p.update(c.chain["select"].p)
        c.p.update(R=1, twin=True)
        return
    s2.p_align2(c, r)
    if c.kind != "select":
        keep = dict(c.p)
        p_align3(c, c.rng(7))
        c.p.update({**keep, "rows": c.p["rows"], "length": c.p["length"]})
    s2.p_panel(c, r)
    screen = (chain == "graph") or (chain == "select" and c.pos == 4)
    if chain == "slab":
        rule = ("any", "end1")[int(r.integers(0, 2))]
    else:
        rule = (0, 0, 0, "end1")[int(r.integers(0, 4))] if c.kind != "select" else 0
    forms = ("dev", "packed") if c.kind == "select_w" else ("bitmap", "dev", "packed")
    c.p.update(form="screen" if screen else forms[int(r.integers(0, len(forms)))],
               T=3 if (chain == "select" and c.pos == 1) else int(r.choice([1, 3])),
               min_gain=int(r.integers(1, 3)), n_forced=int(r.integers(0, 4)), skewed=bool(r.integers(0, 2)), rule=rule)
    if c.kind == "select_depth":
        c.p["R"] = int(r.choice([2, 3]))
    if rule:
        s2.p_scored(c, r)
        c.p["mode"] = rule
    p_split(c)
    if screen:
        c.p.update(screen_chem="ntthal", screen_rule=c.p.get("rule2") or GRAPH_RULES[int(r.integers(0, 2))])
        if chain == "select":                          # ANY alone, END alone or both through the weighted _rule form
            dg, tm = c.p["screen_rule"]
            c.p["screen_rule"] = ((dg, tm), (dg, None), (None, tm))[int(r.integers(0, 3))]
        c.p["rows_n"] = c.p["n_f"] + c.p["n_r"]
    if c.kind == "select":
        c.chain["select"] = c


def p_tolerant3(c, r):
    s2.p_tolerant(c, r)
    c.p["mode"] = "end1"                               # mode 2


def p_graph3(c, r):
    """The graph family.  variant by place: bitmap (a block, row and kind counts), edges (the whole pool as an ordered
    list, once with a capacity below the count and once above), ab (k_a != k_b), any (the bound chain's pool under
    use_any alone).  The square variants of the graph chain share two pools: one per size."""
    chain = chain_of(c)
    if chain == "bound":
        p_bound_shared(c)
        c.p.update(variant="any", rows_n=c.p["n"], optional=int(r.integers(0, 4)))
        return
    variant = {0: "bitmap", 2: "edges", 5: "ab"}[c.pos]
    c.p["variant"] = variant
    if variant == "ab":
        lo, hi = (70, 111) if c.size == "large" else (20, 41)
        ka, kb = ((13, 20), (20, 13))[int(r.integers(0, 2))]
        c.p.update(k_a=ka, k_b=kb, n_a=int(r.integers(lo, hi)), n_b=int(r.integers(lo, hi)), pseed=int(r.integers(1 << 20)))
        c.p["rows_n"] = c.p["n_a"]
        return
    p_graph_pool(c, r)
    n = c.p["n"]
    if variant == "bitmap":
        r0 = int(r.integers(0, n // 4)); r1 = int(r.integers(r0 + n // 2, n + 1))
        c0 = int(r.integers(0, n // 4)); c1 = int(r.integers(c0 + n // 2, n + 1))
        c.p.update(rect=(r0, r1, c0, c1), rows_n=r1 - r0, optional=int(r.integers(0, 4)))
    else:
        c.p.update(rows_n=n, optional=int(r.integers(0, 4)))


def p_graph_pool(c, r):
    """The graph chain's pool of the call's size: 63 / 64 / 65 of the other k, or 150..300 (n % 24 != 0) 13-mers."""
    key = ("pool", c.size)
    if key not in c.chain:
        if c.size == "large":
            n = int(r.integers(150, 301))
            n += n % 24 == 0
            k = 13                                     # the oracle's 20-mer planes cost four times the 13-mers'
        else:
            n, k = int(r.choice([63, 64, 65])), int(GRAPH_KS[int(r.integers(0, 2))])
        c.chain[key] = dict(n=n, k=k, pseed=int(r.integers(1, 1 << 20)))
    c.p.update(c.chain[key])


def p_consumer(c, r):
    """cover_rule, tubes_rule: the host forms that screen the pool under both rules."""
    p_graph_pool(c, r)
    c.p.update(rows_n=c.p["n"], T=int(r.choice([1, 3, 64])))


def p_decide_w(c, r):
    """The bound chain's pool (s2.decide_pool), at a chemistry and threshold at which the windowed instance is usable."""
    if "n" not in c.chain:
        if c.size == "large":
            n = int(r.integers(250, 401))
            n += n % 24 == 0
        else:
            n = int(r.choice([63, 64, 65]))
        c.chain.update(n=n, pool=("skewed", "mixed")[int(r.integers(0, 2))], pseed=int(r.integers(1 << 30)),
                       chem=("ntthal", "primer3")[int(r.integers(0, 2))], thr=float(r.choice([-9000.0, -6000.0])))
    p_bound_shared(c)
    c.p["form"] = "square"
    c.p["window"] = 1 if c.kind == "decide_w" else 0


def p_bound_shared(c):
    if "n" not in c.chain:
        raise AssertionError("the bound chain starts and ends with decide_w")
    c.p.update({key: c.chain[key] for key in ("k", "n", "pool", "pseed", "chem", "thr")})


def p_window_plane(c, r):
    p_bound_shared(c)
    n = c.p["n"]
    if n <= 80:
        rows, cols = (0, n), (0, n)
    else:                                              # a block off the origin, more than one wave of columns
        nr, nc = int(r.integers(30, 49)), int(r.integers(66, 131))
        r0, c0 = int(r.integers(1, n - nr + 1)), int(r.integers(1, n - nc + 1))
        rows, cols = (r0, r0 + nr), (c0, c0 + nc)
    c.p.update(rows=rows, cols=cols)


PARAMS = {"thin": p_thin3, "thin_depth": p_thin3, "thin_w": p_thin3, "thin_thal_depth": p_thin_thal_depth,
          "select": p_sel3, "select_depth": p_sel3, "select_w": p_sel3, "graph": p_graph3, "cover_rule": p_consumer,
          "tubes_rule": p_consumer, "thal": scm.p_bg, "cov_thal": s2.p_cov_thal, "tolerant": p_tolerant3,
          "decide_w": p_decide_w, "decide": p_decide_w, "window_plane": p_window_plane}


def weights_of(r, n_seg: int, mode: str) -> np.ndarray:
    """int64[n_seg]: all ones; or 0 (a fifth), 1, small values and four large ones -- "limit": with one of the large
    ones set so that the total is exactly 2^32 - 1."""
    if mode == "ones":
        return np.ones(n_seg, dtype=np.int64)
    w = r.choice([0, 1, 1, 1, 2, 3, 5, 9, 0, 1], size=n_seg).astype(np.int64)
    big = r.choice(n_seg, size=min(n_seg, 4), replace=False)
    w[big] = r.integers(1_000_000, 100_000_000, size=len(big))
    if mode == "limit":
        w[big[0]] = 0
        w[big[0]] = LIMIT - int(w.sum())
    return w


def d_thin3(c):
    """scm.d_thin (the last three words of a direction repeat its first three).  A depth call forces the last forward
    primer, a later duplicate of an unforced one; a weighted call gets its weights."""
    d = scm.d_thin(c)
    if c.kind == "thin_depth":
        force_last_duplicate(d, c.p["n_f"])
    if c.kind == "thin_w":
        d["w"] = weights_of(c.rng(6), n_segments_of(d["g"], c.p), c.p["weights"])
    return d


def force_last_duplicate(d, n_f: int):
    """The last forward primer, a later duplicate, forced and its earlier copies not: it is the word's representative."""
    last = n_f - 1
    for i in range(last):
        if d["fwd"][i] == d["fwd"][last]:
            d["forced"][i] = 0
    d["forced"][last] = 1


def n_segments_of(g, p) -> int:
    return g.shape[0] * ptm.n_partitions(g.shape[1], p["seg"], p["stride"])


def split_primers(c, d):
    """The primers of the call that has to split a slab: distinct words off the head / tail windows of random
    segments alone (none from elsewhere, none random), 0 or 1 substitution, so that each matches in most rows."""
    r, g, p = c.rng(8), d["g"], c.p
    rows, L = g.shape
    P = ptm.n_partitions(L, p["seg"], p["stride"])
    out, have = ([], []), set()
    for q, n in ((0, p["n_f"]), (1, p["n_r"])):
        while len(out[q]) < n:
            col = int(r.integers(0, P)) * p["stride"] + (p["seg"] - p["W"] if q else 0) + int(r.integers(0, p["W"] - p["k"] + 1))
            w = g[int(r.integers(0, rows)), col:col + p["k"]].tobytes().decode()
            if set(w) - set("ACGT"):
                continue
            if r.integers(0, 2):
                at = int(r.integers(0, p["k"]))
                w = w[:at] + "ACGT"[("ACGT".index(w[at]) + int(r.integers(1, 4))) % 4] + w[at + 1:]
            w = scm.rc(w) if q else w
            if w not in have:
                have.add(w)
                out[q].append(w)
    d["fwd"], d["rev"] = out


def d_thin_thal_depth(c):
    """s2.d_panel with two words of each direction listed twice and the later forward duplicate forced."""
    d = s2.d_panel(c)
    if c.p.get("split"):
        split_primers(c, d)
    d["fwd"][-2:], d["rev"][-2:] = d["fwd"][:2], d["rev"][:2]
    force_last_duplicate(d, c.p["n_f"])
    return d


def d_sel3(c):
    if c.p.get("twin"):
        return c.chain["select"].data()
    d = s2.d_select(c)
    if c.p.get("split"):
        split_primers(c, d)
    if c.kind == "select_w":
        d["w"] = weights_of(c.rng(6), n_segments_of(d["g"], c.p), c.p["weights"])
    return d


def d_graph_pool(c):
    key = ("pooldata", c.p["k"], c.p["n"], c.p["pseed"])
    if key not in c.chain:
        c.chain[key] = {"words": cgm.distinct(cgm.end_pool(c.p["k"], c.p["n"], c.p["pseed"]))}
    return c.chain[key]


def d_graph3(c):
    p = c.p
    if p["variant"] == "any":
        return s2.d_decide(c)
    if p["variant"] != "ab":
        return d_graph_pool(c)
    A, B = cgm.end_pool(p["k_a"], p["n_a"], p["pseed"]), cgm.end_pool(p["k_b"], p["n_b"], p["pseed"] + 1)
    ka, kb = p["k_a"], p["k_b"]
    for j in range(min(8, p["n_a"] // 3, p["n_b"] // 3)):   # oligos that pair with the other pool's 3' ends
        tail = A[j][-min(ka, kb):]
        B[j] = (cgm.rc(tail) + B[j])[:kb]
        tail = B[-1 - j][-min(10, ka, kb):]
        A[-1 - j] = (cgm.rc(tail) + A[-1 - j])[:ka]
    return {"A": A, "B": B}


DATA = {"thin": d_thin3, "thin_depth": d_thin3, "thin_w": d_thin3, "thin_thal_depth": d_thin_thal_depth,
        "select": d_sel3, "select_depth": d_sel3, "select_w": d_sel3, "graph": d_graph3, "cover_rule": d_graph_pool,
        "tubes_rule": d_graph_pool, "thal": scm.d_bg, "cov_thal": s2.d_panel, "tolerant": s2.d_tolerant,
        "decide_w": s2.d_decide, "decide": s2.d_decide, "window_plane": s2.d_decide}


def matrix_shape(c):
    """(primers or seeds padded to 64, segment groups) of a call that fills an incidence matrix; None for the others."""
    if c.kind not in ("thin", "thin_depth", "thin_w", "thin_thal_depth", "cov_thal", "select", "select_depth",
                      "select_w", "tolerant"):
        return None
    p, g = c.p, c.data()["g"]
    n = max(len(s) for s in c.data()["seeds"]) if c.kind == "tolerant" else p["n_f"] + p["n_r"]
    S = group_size(p["W"], p["k"])
    return (n + 63) // 64 * 64, -(-n_segments_of(g, p) // S)


# ---- expected values ---------------------------------------------------------------------------------------------------

u64 = s2.u64


def plane(c, x):
    return np.asarray(x).astype(np.uint8).reshape(c.data()["g"].shape[0], -1)


def mm_incidence(c):
    d, p = c.data(), c.p
    return ptm.incidence(d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], p["M"], p["E"])


def held(c):
    """(held incidence, matches listed) of a call under a thal rule."""
    res = s2.scored_result(c)
    return ttm.held_incidence(res), len(res["matches"])


def split_stats(c, matches: int, n_groups: int, n: int) -> dict:
    """What the model says of the slab loop under the call's work list: the first slab is the whole matrix."""
    cap = SPLIT_CAP if c.option == ("site_list_cap_log2", 12) else 1 << 22
    parts = slab_split_model(0, n_groups, 0, n, matches, cap) if matches > cap else []
    return {"matches": matches, "splits": matches > cap, "parts": len(parts)}


def depth_want(c, I):
    d, p = c.data(), c.p
    sh = dm.shadows(d["fwd"], d["rev"], d["forced"])
    keep, order, gains, d_all, d_kept, counts, rounds, _c0, _c = dm.greedy_depth(I, p["R"], p["min_gain"], d["forced"], sh)
    one = dm.greedy_depth(I, 1, p["min_gain"], d["forced"], sh)
    c.stats.update(kept=int(keep.sum()), kept_at_1=int(one[0].sum()), shadows=int(sh.sum()),
                   thin_segments=int(((d_all > 0) & (d_all < p["R"])).sum()))
    return {"keep": keep, "order": order, "gains": gains, "depth_all": plane(c, d_all), "depth_kept": plane(c, d_kept),
            "counts": counts, "rounds": rounds, "shadows": int(sh.sum())}


def e_thin_depth(c):
    return depth_want(c, mm_incidence(c))


def e_thin_thal_depth(c):
    H, matches = held(c)
    c.stats.update(split_stats(c, matches, matrix_shape(c)[1], c.p["n_f"] + c.p["n_r"]))
    return depth_want(c, H)


def weighted_stats(c, res, ones, w):
    cov = np.asarray(res["covered"]).astype(bool).reshape(-1)
    c.stats.update(picks=len(res["order"]), differs_from_ones=res["order"].tolist() != ones["order"].tolist(),
                   zero_covered=int((cov & (w == 0)).sum()), total=int(w.sum()), weights=c.p["weights"])


def e_thin_w(c):
    d, p = c.data(), c.p
    I = mm_incidence(c)
    res = wm.greedy_weighted(I, d["w"], p["min_gain"], d["forced"])
    flat = ptm.greedy(I, p["min_gain"], d["forced"])
    weighted_stats(c, res, {"order": flat[1]}, d["w"])
    want = {key: res[key] for key in ("keep", "order", "gains", "covered_all", "covered_kept", "weight_all",
                                      "weight_kept", "rounds")}
    want["covered"] = plane(c, res["covered"])
    if p["weights"] == "ones":                         # the unweighted form on the same inputs, straight after
        want.update({"twin.keep": flat[0], "twin.order": flat[1], "twin.gains": flat[2], "twin.covered": plane(c, flat[3]),
                     "twin.covered_all": flat[4], "twin.covered_kept": flat[5], "twin.rounds": flat[6]})
    return want


def panel_graph(c):
    """The conflict matrix of a selection: the caller's, or what the call screens for itself under its rule."""
    d, p = c.data(), c.p
    if p["form"] != "screen":
        return d["b"]
    dg, tm = p["screen_rule"]
    a, e = cgm.random_planes(o, tables(), d["fwd"] + d["rev"], dg if dg is not None else 0.0,
                             tm if tm is not None else 0.0)
    a, e = cgm.enabled(a, e, dg is not None, tm is not None)
    c.stats["screen_kinds"] = cgm.kind_counts(a, e).tolist()
    return cgm.union(a, e).astype(bool)


def sel_incidence(c):
    if not c.p["rule"]:
        return mm_incidence(c)
    H, matches = held(c)
    c.stats.update(split_stats(c, matches, matrix_shape(c)[1], c.p["n_f"] + c.p["n_r"]))
    return H


SELECT_KEYS = ("order", "gains", "keep", "tube", "barred", "covered_all", "covered_kept", "tubes_used", "rounds")


def e_select3(c):
    d, p = c.data(), c.p
    I, B = sel_incidence(c), panel_graph(c)
    res = sm.select(I, B, p["T"], p["min_gain"], d["forced"])
    sm.check_independent(res, B, d["forced"])
    c.graph = B
    c.stats.update(picks=len(res["order"]), edges=int(B.sum()))
    want = {key: res[key] for key in SELECT_KEYS}
    want["covered"] = plane(c, res["covered"])
    return want


def e_select_depth(c):
    d, p = c.data(), c.p
    I, B = sel_incidence(c), panel_graph(c)
    res = sdm.select_depth(I, B, p["R"], p["T"], p["min_gain"], d["forced"])
    sm.check_independent(res, B, d["forced"])
    c.graph = B
    c.stats.update(picks=len(res["order"]), layer2=int((res["layer"] >= 2).sum()), edges=int(B.sum()))
    want = {key: res[key] for key in ("order", "gains", "layer", "keep", "tube", "barred", "counts", "tubes_used",
                                      "rounds", "layers")}
    want.update(depth_all=plane(c, res["depth_all"]), depth_kept=plane(c, res["depth_kept"]))
    if p["R"] == 1:                                    # select's bytes: what the neighbour returns
        flat = sm.select(I, B, p["T"], p["min_gain"], d["forced"])
        for key in ("order", "gains", "keep", "tube", "barred", "tubes_used", "rounds"):
            assert same(flat[key], res[key]), key
        want["as select.covered"] = plane(c, flat["covered"])
    return want


def e_select_w(c):
    d, p = c.data(), c.p
    I, B = sel_incidence(c), panel_graph(c)
    res = wm.select_weighted(I, B, d["w"], p["T"], p["min_gain"], d["forced"])
    sm.check_independent(res, B, d["forced"])
    flat = sm.select(I, B, p["T"], p["min_gain"], d["forced"])
    c.graph = B
    c.stats["edges"] = int(B.sum())
    weighted_stats(c, res, flat, d["w"])
    want = {key: res[key] for key in SELECT_KEYS + ("weight_all", "weight_kept")}
    want["covered"] = plane(c, res["covered"])
    if p["weights"] == "ones":
        want.update({f"twin.{key}": flat[key] for key in SELECT_KEYS})
        want["twin.covered"] = plane(c, flat["covered"])
    return want


def pool_planes(c):
    """(ANY decisions, END decisions) of a graph chain pool under the chain's rule: once per pool."""
    d = c.data()
    if "planes" not in d:
        dg, tm = c.p["rule2"]
        d["planes"] = cgm.random_planes(o, tables(), d["words"], dg, tm)
    return d["planes"]


def kind_stats(c, a, e):
    kinds = cgm.kind_counts(a, e)
    c.stats.update(kinds=kinds.tolist(), all_kinds=bool((kinds > 0).all()))
    return kinds


def e_graph3(c):
    d, p = c.data(), c.p
    v = p["variant"]
    if v == "any":
        _, cf, _ = s2.oracle_pool(c)
        z = np.zeros_like(cf)
        kinds = kind_stats(c, cf, z)
        n = p["n"]
        return {"dev.bitmap": pack_bits(cf), "dev.rc": RC_BASE + cgm.row_counts(cf, z), "dev.kinds": KIND_BASE + kinds}
    if v == "ab":
        a, e = cgm.ab_planes(o, tables(), d["A"], d["B"], -9000.0, 10.0)
        kinds = kind_stats(c, a, e)
        edges = cgm.kind_edges(a, e)
        want = {"dev.bitmap": pack_bits(cgm.union(a, e)), "dev.rc": RC_BASE + cgm.row_counts(a, e),
                "dev.kinds": KIND_BASE + kinds, "dev.count": len(edges)}
        want.update(scm.fields("dev.edges", edges))
        want.update(scm.fields("host.edges", edges))
        return want
    A, E = pool_planes(c)
    if v == "bitmap":
        r0, r1, c0, c1 = p["rect"]
        a, e = cgm.block(A, (r0, r1), (c0, c1)), cgm.block(E, (r0, r1), (c0, c1))
        kinds = kind_stats(c, a, e)
        rcw = np.full(p["n"], RC_BASE, dtype=np.uint32)
        rcw[r0:r1] += cgm.row_counts(a, e)
        return {"dev.bitmap": pack_bits(cgm.union(a, e)), "dev.rc": rcw, "dev.kinds": KIND_BASE + kinds,
                "host.bitmap": pack_bits(cgm.union(A, E)), "host.rc": cgm.row_counts(A, E),
                "host.kinds": cgm.kind_counts(A, E)}
    kinds = kind_stats(c, A, E)
    edges = cgm.kind_edges(A, E)
    blocked, rcb = cgm.by_blocks(A, E, 7)              # the model's own statement that row blocks change nothing
    assert same(blocked, edges) and same(rcb, cgm.row_counts(A, E))
    low = len(edges) // 2
    c.stats.update(edges=len(edges), truncated_at=low)
    want = {"dev.count": len(edges), "dev.rc": RC_BASE + cgm.row_counts(A, E), "dev.kinds": KIND_BASE + kinds,
            "dev.bitmap": pack_bits(cgm.union(A, E)), "low.count": len(edges)}
    want.update(scm.fields("dev.edges", edges))
    want.update(scm.fields("low.edges", edges[:low]))
    return want


def e_cover_rule(c):
    d = c.data()
    A, E = pool_planes(c)
    deleted, rounds = crm.round_cover(crm.symmetrise(cgm.union(A, E).astype(bool)), crm.lex_rank(d["words"]))
    c.stats.update(rounds=rounds, deleted=int(deleted.sum()))
    return {"deleted": deleted, "rounds": rounds}


def e_tubes_rule(c):
    d = c.data()
    A, E = pool_planes(c)
    want = scm.tubes_want("host", crm.symmetrise(cgm.union(A, E).astype(bool)), crm.lex_rank(d["words"]), c.p["T"])
    c.stats.update(used=want["host.used"], unplaced=want["host.unplaced"])
    return want


def e_decide_w(c):
    _, cf, _ = s2.oracle_pool(c)
    c.stats.update(conflicts=int(cf.sum()), pairs=cf.size)
    return {"bits": cf, "rc": cf.sum(1).astype(np.uint32)}


def e_window_plane(c):
    """The windowed instance's value of every pair of the block (tests/pair_bound_window_model.py plane_model)."""
    import msspe_amd as m
    d, p = c.data(), c.p
    pk = window_tables(m, None, chem_obj(m, p["chem"]), p["thr"])
    assert pk["usable"] == 1 and pk["window"]["usable"] == 1, "the chain's chemistry and threshold run the window"
    rows, cols = d["pool"][p["rows"][0]:p["rows"][1]], d["pool"][p["cols"][0]:p["cols"][1]]
    ur, ri = np.unique(np.array(rows), return_inverse=True)
    uc, ci = np.unique(np.array(cols), return_inverse=True)
    pick, vmin, vmax = window_plane_model(pk, list(ur), list(uc))
    assert vmin == NONE or (pk["lo"] <= vmin and vmax <= pk["hi"])
    model = np.where(pick == NONE, np.inf, (pick + pk["init"]) * pk["unit"])[np.ix_(ri, ci)]
    cut = m.g_cut(p["thr"])
    fin = np.isfinite(model)
    c.stats.update(finite=int(fin.sum()), culled=int((model[fin] > cut).sum()), unit=float(pk["unit"]))
    return {"window.model": model, "window.unit": float(pk["unit"])}


EXPECT = {"thin": scm.e_thin, "thin_depth": e_thin_depth, "thin_w": e_thin_w, "thin_thal_depth": e_thin_thal_depth,
          "select": e_select3, "select_depth": e_select_depth, "select_w": e_select_w, "graph": e_graph3,
          "cover_rule": e_cover_rule, "tubes_rule": e_tubes_rule, "thal": scm.e_thal, "cov_thal": s2.e_cov_thal,
          "tolerant": s2.e_tolerant, "decide_w": e_decide_w, "decide": e_decide_w, "window_plane": e_window_plane}
MODEL_ONLY = ("window.model", "window.unit")           # what a runner reads of `want` itself


def expect(c: Call) -> dict:
    """The expected outputs of a call (computed once), and c.stats: what the non-triviality counters read."""
    if c._want is None:
        c.stats = {}
        c._want = EXPECT[c.kind](c)
    return c._want


def counters(calls) -> dict:
    """What keeps a session from being vacuous, from the expected values of its calls (expect() has run on each)."""
    of = lambda *kinds: [c.stats for c in calls if c.kind in kinds]
    return {
        "graph_all_three_kinds": any(s.get("all_kinds") for s in of("graph")),
        "edge_list_truncated": any(0 < s.get("truncated_at", 0) < s["edges"] for s in of("graph") if "edges" in s),
        "depth_keeps_more_and_has_shadows": any(s["kept"] > s["kept_at_1"] and s["shadows"] >= 1
                                                for s in of("thin_depth", "thin_thal_depth")),
        "weights_change_the_picks": any(s["differs_from_ones"] for s in of("thin_w", "select_w")),
        "zero_weight_segment_covered": any(s["zero_covered"] >= 1 for s in of("thin_w", "select_w")),
        "select_depth_layer_2": any(s["layer2"] >= 1 for s in of("select_depth")),
        "slab_splits": any(s.get("splits") and s.get("parts", 0) >= 2 for s in of("thin_thal_depth", "select_w", "tolerant")),
        "decide_some_conflicts": any(0 < s["conflicts"] < s["pairs"] for s in of("decide_w")),
        "window_culls": any(s["culled"] >= 1 for s in of("window_plane")),
    }


# ---- running a call on an engine --------------------------------------------------------------------------------------

kmer_opt = s2.kmer_opt


def r_thin_depth(c, eng, m, dv, want):
    p, d = c.p, c.data()
    if c.kind == "thin_depth":
        res = eng.panel_thin_depth(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"], p["R"], p["min_gain"],
                                   d["forced"], p["form"])
    else:
        res = eng.panel_thin_thal_depth(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"],
                                        chem_obj(m, p["chem"]), p["mode"], p["thr"], p["R"], p["min_gain"], d["forced"],
                                        p["form"])
    got = dict(zip(("keep", "order", "gains", "depth_all", "depth_kept", "counts"), res))
    got.update(rounds=eng.info("panel_thin_rounds"), shadows=eng.info("panel_thin_depth_shadows"))
    return got, split_problems(c, eng, "panel_thin_thal_redone") if c.kind == "thin_thal_depth" else []


def split_problems(c, eng, key):
    """Where the model says the first slab overran the work list, the pass has to have split one."""
    if c.stats.get("splits") and eng.info(key) <= 0:
        return [f"{key} is 0, the model lists {c.stats['matches']} matches for a work list of {SPLIT_CAP}"]
    return []


THIN_KEYS = ("keep", "order", "gains", "covered", "covered_all", "covered_kept")


def r_thin_w(c, eng, m, dv, want):
    p, d = c.p, c.data()
    res = eng.panel_thin_weighted(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"], d["w"], p["min_gain"],
                                  d["forced"], p["form"])
    got = dict(zip(THIN_KEYS + ("weight_all", "weight_kept"), res))
    got["rounds"] = eng.info("panel_thin_rounds")
    problems = []
    if p["weights"] == "ones":
        flat = eng.panel_thin(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], p["M"], p["E"], p["min_gain"], d["forced"],
                              p["form"])
        got.update({f"twin.{key}": v for key, v in zip(THIN_KEYS, flat)})
        got["twin.rounds"] = eng.info("panel_thin_rounds")
        problems += [f"all ones: {key} differs from the unweighted call's" for key in THIN_KEYS + ("rounds",)
                     if not same(got[key], got[f"twin.{key}"])]
    return got, problems


def sel_rule(c, m):
    p = c.p
    return m.seed_rule(p["M"], p["E"], p["rule"], chem_obj(m, p["chem"]), p["thr"]) if p["rule"] else \
        m.seed_rule(p["M"], p["E"])


def sel_graph_args(c, m):
    """(bitmap, form, keyword arguments) of a selection: the caller's bitmap, or the screen under the call's rule."""
    p, d = c.p, c.data()
    if p["form"] != "screen":
        return sm.pack_bitmap(d["b"]), p["form"], {}
    dg, tm = p["screen_rule"]
    return None, "screen", dict(chem=chem_obj(m, p["screen_chem"]), threshold=dg, end_tm_threshold=tm)


def guarantees(res, c, problems):
    try:
        sm.check_independent(res, c.graph, c.data()["forced"])
    except AssertionError as e:
        problems.append(f"the device's result breaks a guarantee of the selection: {e!r}")


def r_select3(c, eng, m, dv, want):
    p, d = c.p, c.data()
    bitmap, form, kw = sel_graph_args(c, m)
    res = eng.panel_select(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], sel_rule(c, m), bitmap, p["T"], p["min_gain"],
                           False, d["forced"], form, **kw)
    got = dict(res)
    got["rounds"] = eng.info("panel_select_rounds")
    c.chain["select got"] = got
    problems = []
    guarantees(res, c, problems)
    if "twin got" in c.chain:                          # a reversed chain: select_depth at R = 1 ran just before
        problems += twin_problems(c.chain["twin got"], got)
    return got, problems


def twin_problems(one, flat):
    """select_depth at R = 1 against the neighbouring select on the same inputs: select's bytes."""
    out = [f"R = 1: {key} differs from the neighbouring select's" for key in
           ("order", "gains", "keep", "tube", "barred", "tubes_used", "rounds") if not same(one[key], flat[key])]
    if not same(one["as select.covered"], flat["covered"]):
        out.append("R = 1: depth_kept != 0 differs from the neighbouring select's covered")
    return out


def r_select_depth(c, eng, m, dv, want):
    p, d = c.p, c.data()
    bitmap, form, kw = sel_graph_args(c, m)
    if form == "screen" and kw["threshold"] is None:
        raise AssertionError("the depth forms that screen themselves take an ANY threshold")
    res = eng.panel_select_depth(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], sel_rule(c, m), p["R"], bitmap, p["T"],
                                 p["min_gain"], False, d["forced"], form, **kw)
    got = dict(res)
    got.update(rounds=eng.info("panel_select_rounds"), layers=eng.info("panel_select_depth_layers"))
    problems = split_problems(c, eng, "panel_thin_thal_redone") if p["rule"] else []
    guarantees(res, c, problems)
    if p["R"] == 1:
        got["as select.covered"] = (res["depth_kept"] != 0).astype(np.uint8)
        if p.get("twin"):                              # the neighbour's own bytes: it ran just before, or runs next
            c.chain["twin got"] = got
            if "select got" in c.chain:
                problems += twin_problems(got, c.chain["select got"])
    return got, problems


def r_select_w(c, eng, m, dv, want):
    p, d = c.p, c.data()
    bitmap, form, kw = sel_graph_args(c, m)
    res = eng.panel_select_weighted(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], sel_rule(c, m), d["w"], bitmap, p["T"],
                                    p["min_gain"], False, d["forced"], form, **kw)
    got = dict(res)
    got["rounds"] = eng.info("panel_select_rounds")
    problems = split_problems(c, eng, "panel_thin_thal_redone") if p["rule"] else []
    guarantees(res, c, problems)
    if p["weights"] == "ones":                         # the unweighted form on the same inputs, straight after
        if form == "screen" and kw["threshold"] is None:
            c.dropped = [key for key in want if key.startswith("twin.")]   # END alone has no unweighted form
            return got, problems
        flat = eng.panel_select(d["g"], kmer_opt(m, p), d["fwd"], d["rev"], sel_rule(c, m), bitmap, p["T"],
                                p["min_gain"], False, d["forced"], form, **kw)
        got.update({f"twin.{key}": v for key, v in flat.items()})
        got["twin.rounds"] = eng.info("panel_select_rounds")
        problems += [f"all ones: {key} differs from the unweighted call's" for key in SELECT_KEYS + ("covered",)
                     if not same(got[key], got[f"twin.{key}"])]
    return got, problems


EDGE = cgm.KIND_EDGE


def graph_outputs(c, dv, n_rows, rc_len, words, optional, cap=None):
    """Dirty device outputs of a graph call: row counts at RC_BASE, kind counts at KIND_BASE, the bitmap and the edge
    list as sentinels.  optional: 1 drops the row counts, 2 the kind counts, 3 the bitmap (with an edge list only)."""
    out = {"rc": 0 if optional == 1 else dv.put(np.concatenate([np.full(rc_len, RC_BASE, dtype=np.uint32),
                                                                 sentinel(0, np.uint32)])),
           "kinds": 0 if optional == 2 else dv.put(np.concatenate([KIND_BASE, sentinel(0, np.uint64)])),
           "bm": 0 if optional == 3 and cap is not None else dv.put(sentinel(n_rows * words, np.uint64))}
    if cap is not None:
        out["edges"], out["count"] = dv.put(sentinel(cap, EDGE)), dv.put(np.full(1, 123, dtype=np.uint64))
    return out


def graph_read(dv, out, n_rows, rc_len, words, prefix, cap, got, problems):
    if out["rc"]:
        rcw = dv.get(out["rc"], rc_len + GUARD, np.uint32)
        guard_ok(rcw, rc_len, "row counts", problems)
        got[f"{prefix}.rc"] = rcw[:rc_len]
    if out["kinds"]:
        kinds = dv.get(out["kinds"], 3 + GUARD, np.uint64)
        guard_ok(kinds, 3, "kind counts", problems)
        got[f"{prefix}.kinds"] = kinds[:3]
    if out["bm"]:
        bm = dv.get(out["bm"], n_rows * words + GUARD, np.uint64)
        guard_ok(bm, n_rows * words, "bitmap", problems)
        got[f"{prefix}.bitmap"] = bm[:n_rows * words].reshape(n_rows, words)
    if cap is not None:
        cnt = int(dv.get(out["count"], 1, np.uint64)[0])
        rec = dv.get(out["edges"], cap + GUARD, EDGE)
        guard_ok(rec, min(cnt, cap), f"{prefix} edge list", problems)
        got[f"{prefix}.count"] = cnt
        got.update(scm.fields(f"{prefix}.edges", rec[:min(cnt, cap)]))


def drop_optional(want, prefix, out):
    """The expected values without those of an output the call passed as NULL."""
    gone = [f"{prefix}.{name}" for name, key in (("rc", "rc"), ("kinds", "kinds"), ("bitmap", "bm")) if not out[key]]
    return {key: v for key, v in want.items() if key not in gone}


def r_graph3(c, eng, m, dv, want):
    p, d = c.p, c.data()
    v = p["variant"]
    got, problems = {}, []
    if v == "ab":
        chem, rule = m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0)
        A, B, n_a, n_b = d["A"], d["B"], p["n_a"], p["n_b"]
        words = (n_b + 63) // 64
        d_a, d_b = dv.put(m.pack_oligos(A)), dv.put(m.pack_oligos(B))
        cap = want["dev.count"] + 8
        out = graph_outputs(c, dv, n_a, n_a, words, 0, cap)
        eng.conflict_graph_ab_edges_dev(d_a, n_a, p["k_a"], d_b, n_b, p["k_b"], chem, rule, (0, n_a), (0, n_b),
                                        out["edges"], cap, out["count"], out["rc"], out["bm"], out["kinds"])
        eng.synchronize()
        graph_read(dv, out, n_a, n_a, words, "dev", cap, got, problems)
        try:
            edges, _ = eng.conflict_graph_ab_edges(A, B, chem, rule, capacity=cap)
            got.update(scm.fields("host.edges", edges))
        except m.MsspeError as e:                      # more edges than the model has: a difference, not a crash
            problems.append(f"host edge list: {e}")
        return got, problems
    if v == "any":
        chem, rule = chem_obj(m, p["chem"]), m.ConflictRule.of(p["thr"], None)
        pool, n = d["pool"], p["n"]
    else:
        chem, rule = m.Chem.ntthal(), m.ConflictRule.of(*p["rule2"])
        pool, n = d["words"], p["n"]
    d_pool = dv.put(m.pack_oligos(pool))
    k = p["k"]
    if v in ("any", "bitmap"):
        r0, r1, c0, c1 = p["rect"] if v == "bitmap" else (0, n, 0, n)
        words = (c1 - c0 + 63) // 64
        out = graph_outputs(c, dv, r1 - r0, n, words, p["optional"])
        eng.conflict_graph_dev(d_pool, n, k, chem, rule, (r0, r1), (c0, c1), out["rc"], out["bm"], out["kinds"])
        eng.synchronize()
        graph_read(dv, out, r1 - r0, n, words, "dev", None, got, problems)
        if v == "bitmap":
            host = eng.conflict_graph(pool, chem, rule)
            got.update({"host.bitmap": host["bitmap"], "host.rc": host["row_conflicts"], "host.kinds": host["kind_counts"]})
        c.dropped = [key for key in want if key not in drop_optional(want, "dev", out)]
        return got, problems
    words = (n + 63) // 64
    # the truncated list alone (every other output NULL), then the whole list beside the call's other outputs
    for prefix, cap, optional in (("low", want["low.edges.a"].size, None), ("dev", want["dev.count"] + 8, p["optional"])):
        out = graph_outputs(c, dv, n, n, words, 3 if optional is None else optional, cap)
        if optional is None:
            out.update(rc=0, kinds=0)
        eng.conflict_graph_edges_dev(d_pool, n, k, chem, rule, (0, n), (0, n), out["edges"], cap, out["count"],
                                     out["rc"], out["bm"], out["kinds"])
        eng.synchronize()
        graph_read(dv, out, n, n, words, prefix, cap, got, problems)
        if prefix == "dev":
            c.dropped = [key for key in want if key.startswith("dev.") and key not in drop_optional(want, "dev", out)]
    return got, problems


def r_cover_rule(c, eng, m, dv, want):
    p, d = c.p, c.data()
    dg, tm = p["rule2"]
    deleted = eng.conflict_cover(d["words"], m.Chem.ntthal(), dg, end_tm_threshold=tm)
    return {"deleted": deleted, "rounds": eng.info("cover_rounds")}, []


def r_tubes_rule(c, eng, m, dv, want):
    p, d = c.p, c.data()
    dg, tm = p["rule2"]
    tube, used, unplaced = eng.conflict_tubes(d["words"], m.Chem.ntthal(), dg, p["T"], end_tm_threshold=tm)
    return {"host.tube": tube, "host.used": used, "host.unplaced": unplaced, "host.rounds": eng.info("tube_rounds")}, []


def r_decide_w(c, eng, m, dv, want):
    """The decision-only square screen with the bound stage on and pair_bound_window at the call's value."""
    p, d = c.p, c.data()
    chem, pool, n = chem_obj(m, p["chem"]), d["pool"], p["n"]
    own = {"pair_bound": 1, "pair_bound_window": p["window"]}
    if c.option:
        own.pop(c.option[0], None)
    for key, v in own.items():
        eng.set_option(key, v)
    try:
        eng.pair_stage_stats()
        out = eng.cross_dimer(pool, chem, p["thr"], want_dg=False)
        stats = eng.pair_stage_stats()
    finally:
        for key in own:
            eng.set_option(key, "auto")
    problems = []
    if not c.option:                                   # the counters say which instance ran
        ran = stats["bound_window_survivors"] > 0
        if p["window"] and not ran and stats["bound_survivors"] > 0:
            problems.append("pair_bound_window 1: the packed instance ran")
        if not p["window"] and ran:
            problems.append("pair_bound_window 0: the windowed instance ran")
    return {"bits": bits(out["bitmap"], n), "rc": out["row_conflicts"]}, problems


def r_window_plane(c, eng, m, dv, want):
    """The windowed plane against the model as tests/test_gpu_pair_bound_window.py check_planes compares it: a finite
    value is the model's, +-inf stand where the packed instance's plane has them, no value above the packed one's."""
    p, d = c.p, c.data()
    chem, pool, n = chem_obj(m, p["chem"]), d["pool"], p["n"]
    rows, cols = p["rows"], p["cols"]
    R, Cc = rows[1] - rows[0], cols[1] - cols[0]
    problems, planes = [], {}
    d_pool = dv.put(m.pack_oligos(pool))
    for name, call in (("window", eng.cross_dimer_bound_window_dev), ("packed", eng.cross_dimer_bound_packed_dev)):
        d_b = dv.put(sentinel(R * Cc, np.float64))
        call(d_pool, n, p["k"], chem, p["thr"], rows, cols, d_b)
        b = dv.get(d_b, R * Cc + GUARD, np.float64)
        guard_ok(b, R * Cc, f"{name} plane", problems)
        planes[name] = b[:R * Cc].reshape(R, Cc).copy()
    b, packed = planes["window"], planes["packed"]
    s2.check_bounded(b, want["window.model"], "windowed plane", problems)
    for v in (-np.inf, np.inf):
        if not np.array_equal(b == v, packed == v):
            problems.append(f"windowed plane: {v} at other pairs than in the packed plane")
    fin = np.isfinite(b) & np.isfinite(packed)
    if (b[fin] > packed[fin]).any() or (np.mod(b[np.isfinite(b)], want["window.unit"]) != 0).any():
        problems.append("windowed plane: a value above the packed instance's, or off the unit")
    return {name: u64(x) for name, x in planes.items()}, problems


def r_thal3(c, eng, m, dv, want):
    got, problems = scm.r_thal(c, eng, m, dv, want)
    if c.option == ("site_list_cap_log2", 12) and len(want["sites.pos"]) > SPLIT_CAP and \
            eng.info("background_thal_redone") <= 0:
        problems.append(f"background_thal_redone is 0 at {len(want['sites.pos'])} sites for a work list of {SPLIT_CAP}")
    return got, problems


RUN = {"thin": scm.r_thin, "thin_depth": r_thin_depth, "thin_w": r_thin_w, "thin_thal_depth": r_thin_depth,
       "select": r_select3, "select_depth": r_select_depth, "select_w": r_select_w, "graph": r_graph3,
       "cover_rule": r_cover_rule, "tubes_rule": r_tubes_rule, "thal": r_thal3, "cov_thal": s2.r_cov_thal,
       "tolerant": s2.r_tolerant, "decide_w": r_decide_w, "decide": r_decide_w, "window_plane": r_window_plane}


def run_call(c: Call, eng, m, want) -> tuple[dict, list]:
    """One call on the engine, under its option if it has one (restored whatever happens): (outputs, problems)."""
    dv = Device(eng)
    c.dropped = []
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
    engine_s = 0.0
    for c in calls[:last + 1]:
        t0 = time.perf_counter()
        want = expect(c)
        t1 = time.perf_counter()
        got, problems = run_call(c, eng, m, want)
        t2 = time.perf_counter()
        engine_s += t2 - t1
        if c.index < 3:
            first[c.index] = image(got)
        checked = {key: v for key, v in want.items() if key not in MODEL_ONLY and key not in c.dropped}
        bad = [] if only is not None and c.index != only else differences(got, checked) + problems
        if c.kind == "decide_w" and not bad:
            if squares.setdefault(c.block, image(got)) != image(got):
                bad.append("the bound chain's last screen differs from its first")
        log(f"{c.describe()} model {t1 - t0:.2f} s engine {t2 - t1:.2f} s {c.stats} {'ok' if not bad else bad}")
        failures += [f"{c.describe()}: {b}" for b in bad]
    if only is None:
        for c in calls[:3]:
            t1 = time.perf_counter()
            got, problems = run_call(c, eng, m, expect(c))
            engine_s += time.perf_counter() - t1
            same_bytes = image(got) == first[c.index]
            log(f"replay of call {c.index} ({c.kind}) {'identical' if same_bytes else 'DIFFERS'}")
            if not same_bytes:
                failures.append(f"{c.describe()}: replay at the end of the session differs from the first run")
            failures += [f"{c.describe()} (replay): {b}" for b in problems]
    log(f"seed {seed}: engine {engine_s:.2f} s in all")
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
        many = c.kind in ("thin_depth", "thin_thal_depth", "select_depth", "thin_w", "select_w", "graph")
        out.add(("kind", c.kind, c.size) if many else ("kind", c.kind))
        if c.kind in KS and c.kind in NEW_FAMILIES:
            out.add(("k", c.kind, p["k"]))
        if c.option:
            name, value = c.option
            out.add(("option", name, "rows" if name == "conflict_graph_block_rows" else value))
        out.add(("chain", c.block))
        if c.kind == "graph":
            out.add(("graph", p["variant"]))
            out.add(("graph k", p.get("k", (p.get("k_a"), p.get("k_b")))) if p["variant"] != "any" else ("graph", "any"))
            if p["variant"] in ("bitmap", "edges", "any"):
                out.add(("graph optional", p["optional"]))
            if p["variant"] in ("bitmap", "edges"):
                out.add(("graph n", p["n"] if p["n"] <= 65 else "large"))
        if c.kind in ("cover_rule", "tubes_rule"):
            out.add(("graph n", p["n"] if p["n"] <= 65 else "large"))
        if c.kind == "tubes_rule":
            out.add(("T", p["T"]))
        if c.kind in ("thin_depth", "thin_thal_depth", "select_depth"):
            out.add(("R", c.kind, p["R"]))
        if c.kind in ("thin_w", "select_w"):
            out.add(("weights", c.kind, p["weights"]))
        if c.kind in ("thin_depth", "thin_thal_depth", "thin_w", "select_depth", "select_w"):
            out.add(("form", c.kind, p["form"]))
            out |= {("primers", p["n_f"]), ("primers", p["n_r"])} & {("primers", x) for x in (63, 64, 65)}
            out.add(("window", p["seg"]))
            if group_size(p["W"], p["k"]) > 1 and n_segments_of_shape(p) % group_size(p["W"], p["k"]) == 1:
                out.add(("last group of one", group_size(p["W"], p["k"])))
        if c.kind in ("select_depth", "select_w"):
            out.add(("select incidence", "thal" if p["rule"] else "mismatch"))
            if p["form"] == "screen":
                dg, tm = p["screen_rule"]
                out.add(("screen rule", dg is not None, tm is not None))
        if c.kind == "decide_w":
            out.add(("decide n", p["n"] if p["n"] <= 65 else "large"))
            out.add(("decide pool", p["pool"]))
    return out


def n_segments_of_shape(p) -> int:
    """rows * P from the drawn shape alone (the generator adds less than a stride to a length that divides)."""
    return p["rows"] * ptm.n_partitions(p["length"], p["seg"], p["stride"])


def required() -> set:
    many = ("thin_depth", "thin_thal_depth", "select_depth", "thin_w", "select_w", "graph")
    out = {("kind", f, s) for f in many if f != "thin_depth" for s in ("large", "small")}
    out |= {("kind", "thin_depth", s) for s in ("large", "small")}
    out |= {("kind", f) for f in ("cover_rule", "tubes_rule", "window_plane", "decide_w", "decide", "thin", "select",
                                  "thal", "cov_thal", "tolerant")}
    out |= {("k", f, k) for f in NEW_FAMILIES if f in KS for k in KS[f]}
    out |= {("option", name, value) for name, value, _ in OPTIONS}
    out |= {("chain", f"{name}:{d}") for name in CHAINS for d in ("fwd", "rev")}
    out |= {("graph", v) for v in ("bitmap", "edges", "ab", "any")}
    out |= {("graph k", k) for k in GRAPH_KS + ((13, 20), (20, 13))}
    out |= {("graph optional", x) for x in (0, 1, 2, 3)} | {("graph n", x) for x in (63, 64, 65, "large")}
    out |= {("T", t) for t in (1, 3, 64)}
    out |= {("R", "thin_depth", x) for x in (1, 2, 3)} | {("R", f, x) for f in ("thin_thal_depth", "select_depth")
                                                          for x in (2, 3)} | {("R", "select_depth", 1)}
    out |= {("weights", f, x) for f in ("thin_w", "select_w") for x in WEIGHT_MODES}
    out |= {("form", f, x) for f in ("thin_depth", "thin_thal_depth", "thin_w") for x in ("host", "dev", "packed")}
    out |= {("form", "select_depth", x) for x in ("bitmap", "dev", "packed", "screen")}
    out |= {("form", "select_w", x) for x in ("dev", "packed", "screen")}
    out |= {("primers", x) for x in (63, 64, 65)} | {("window", w[0]) for w in WINDOWS} | {("last group of one", 53)}
    out |= {("select incidence", x) for x in ("thal", "mismatch")}
    out |= {("screen rule", True, True), ("screen rule", True, False), ("screen rule", False, True)}
    out |= {("decide n", x) for x in (63, 64, 65, "large")} | {("decide pool", x) for x in ("skewed", "mixed")}
    return out
