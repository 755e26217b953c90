"""The session campaign (tools/random_campaign_session.py, tests/test_gpu_session_campaign.py): schedules of randomised
calls over the entry points added after the first campaigns -- END, pool against pool and mixed lengths, the thal record,
seeded stage A, coverage within M mismatches, panel thinning, the device cover and tube split, the background family --
all on ONE msspe_ctx, and what every call has to return.

Expected values come from the CPU oracle (oracle/pyoracle.py) and the numpy models under tests/ alone, never from the
engine.  This module holds no GPU code and does not import torch or the product package: run_session() is handed the
engine and the package by its caller; schedule(), expect() and counters() need neither (the CPU-only mode).

Schedule of a seed (schedule()): the four chains of neighbours that share work areas of the context
    cover -> tubes -> cover                              (tubes lives in cover's buffers)
    sites -> thal -> flank -> amplicons -> flank 0       (site_work / amp_work, one set of streams)
    coverage -> thin -> coverage                         (mm_cov, thin)
    ANY -> END -> background thal "any"                  (one chemistry and one numeric threshold: the three cut kinds)
each forwards or reversed, one more call of every family a chain holds once, and two calls of one family outside the
chains (pool against pool, the thal record, stage A), in shuffled order.  Every family is called at the large and at the
small end of its range ("first_large": the large call comes first), with different k where it has one.  The chains take
14 calls and the second calls 4, so a session has 20 calls -- not the 14 to 18 the campaign was first planned with, which
the four chains and two calls per family do not fit into; it ends by repeating its first three.  With probability
1/4 a call runs under one non-default engine option that its family reads, which no expected value depends on."""
from __future__ import annotations

import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import background_amplicon_model as bam
import background_flank_model as bfm
import background_model as bgm
import background_thal_model as btm
import cover_round_model as crm
import coverage_mm_model as cm
import panel_thin_model as ptm
import pyoracle as o
import tube_round_model as trm
from stage_a_seeded_model import SeededModel

# the seeds of the suite (tests/test_session_campaign_model.py holds what they have to cover together)
SEEDS = (1, 15, 33, 43, 44, 53, 68, 71)

FAMILIES = ("any", "end", "ab", "detail", "stage_a", "coverage", "thin", "cover_tubes", "bg_sites", "bg_thal")
FREE_FAMILIES = ("ab", "detail", "stage_a")
CHAINS = {
    "cover": (("cover_tubes", "cover"), ("cover_tubes", "tubes"), ("cover_tubes", "cover")),
    "background": (("bg_sites", "sites"), ("bg_thal", "thal"), ("bg_thal", "flank"), ("bg_thal", "amplicons"),
                   ("bg_thal", "flank0")),
    "coverage": (("coverage", "coverage"), ("thin", "thin"), ("coverage", "coverage")),
    "chem": (("any", "any"), ("end", "end"), ("bg_thal", "thal_any")),
}
KS = {
    "any": (9, 13, 14, 15, 16, 20), "end": (5, 13, 17, 25), "ab": ((13, 20), (20, 13), (16, 22), (9, 31)),
    "detail": (3, 13, 24, 32), "stage_a": (5, 8, 13, 16), "coverage": (5, 8, 13, 16), "thin": (5, 8, 13, 16),
    "bg_sites": (8, 13, 20, 24), "bg_thal": (8, 13, 20, 24),
}
WINDOWS = ((500, 250, 50), (200, 100, 40), (60, 30, 30))
# option -> (non-default value, default), and per family the options an entry point of it reads (csrc/capi.cpp)
OPTIONS = {
    "pair_kernel": ("f64", "auto"), "force_generic": (1, 0), "wave_kernel": (0, 1), "split_list": (0, 1),
    "short_chain": (0, 1), "list_cap_log2": (20, 0), "site_list_cap_log2": (12, 22),
    "amplicon_keys_cap_log2": (10, 20), "stage_a_graph": (0, 1), "stage_a_candidates": (0, 1),
}
PAIR_OPTIONS = ("pair_kernel", "force_generic", "wave_kernel", "split_list", "short_chain", "list_cap_log2")
OPTIONS_OF = {
    "any": PAIR_OPTIONS, "end": ("force_generic", "wave_kernel", "list_cap_log2"), "ab": PAIR_OPTIONS,
    "cover_tubes": PAIR_OPTIONS, "stage_a": ("stage_a_graph", "stage_a_candidates"),
    "bg_thal": ("site_list_cap_log2", "amplicon_keys_cap_log2", "force_generic", "wave_kernel", "list_cap_log2"),
}
CHEMS = {"ntthal": ("ntthal", {}), "primer3": ("primer3", {}), "ntthal37": ("ntthal", dict(temp_c=37.0))}
RC_BASE = 5                       # row_conflicts is added to: the buffer starts at this
GUARD = 64                        # bytes / elements of sentinel behind every device output
FILL = 0xA5
THAL_DETAIL_DTYPE = np.dtype([("dS", np.float64), ("dH", np.float64), ("dG", np.float64), ("t", np.float64),
                              ("no_structure", np.int32), ("n_pairs", np.int32),
                              ("ps1", np.uint8, (32,)), ("ps2", np.uint8, (32,))])
_COMP = str.maketrans("ACGT", "TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rc(s: str) -> str:
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n: int) -> str:
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = o.Tables()
    return _tables


def chem_args(name):
    base, kw = CHEMS[name]
    return o.ntthal_args(**kw) if base == "ntthal" else o.p3_args(**kw)


def chem_obj(m, name):
    base, kw = CHEMS[name]
    return m.Chem.ntthal(**kw) if base == "ntthal" else m.Chem.primer3(**kw)


# ---- the schedule -----------------------------------------------------------------------------------------------------

class Call:
    def __init__(self, seed, index, family, kind, size, block):
        self.seed, self.index, self.family, self.kind, self.size, self.block = seed, index, family, kind, size, block
        self.p = {}               # every drawn parameter (what the failure message prints)
        self.option = None        # (name, value) set for this call alone
        self.shared = None        # the chain's dict: inputs and model results its calls have in common
        self._data = None
        self._want = None

    def rng(self, salt=0):
        return np.random.default_rng([self.seed, self.index, salt])

    def data(self):
        if self._data is None:
            self._data = DATA[self.kind](self)
        return self._data

    def describe(self):
        opt = f" option {self.option[0]}={self.option[1]}" if self.option else ""
        return (f"seed {self.seed} call {self.index} family {self.family} ({self.kind}, {self.size}, {self.block}) "
                f"{self.p}{opt}")


def schedule(seed: int) -> list[Call]:
    """The calls of a session, without the replay of the first three.  Deterministic per seed."""
    rng = np.random.default_rng([seed, 0x5E5510])
    first_large = bool(rng.random() < 0.75)
    free = FREE_FAMILIES[int(rng.integers(0, 3))]
    blocks = []
    for name, chain in CHAINS.items():
        fwd = bool(rng.integers(0, 2))
        blocks.append((f"{name}:{'fwd' if fwd else 'rev'}", list(chain if fwd else chain[::-1])))
    singles = [("any", "any"), ("end", "end"), ("bg_sites", "sites"), ("thin", "thin"), (free, free), (free, free)]
    blocks += [("single", [s]) for s in singles]
    order = rng.permutation(len(blocks))
    blocks = [blocks[i] for i in order]
    # the background chain runs on one set of streams, so it is large or small as a whole: its two partners (the single
    # sites call and the chem chain, which holds the other thal call) go to one side of it
    side = int(rng.integers(0, 2))
    moved = [b for b in blocks if b[1] == [("bg_sites", "sites")] or b[0].startswith("chem:")]
    blocks = [b for b in blocks if b not in moved]
    at = next(i for i, b in enumerate(blocks) if b[0].startswith("background:"))
    for b in moved:
        lo, hi = (0, at) if side == 0 else (at + 1, len(blocks))
        pos = int(rng.integers(lo, hi + 1))
        blocks.insert(pos, b)
        at += pos <= at
    calls, seen = [], {}
    bg_size = None
    for name, items in blocks:
        for family, kind in items:
            if name.startswith("background:"):
                if bg_size is None:
                    before = max(seen.get("bg_sites", 0), seen.get("bg_thal", 0))
                    bg_size = ("large" if first_large else "small") if before == 0 else \
                        ("small" if first_large else "large")
                size = bg_size
            elif kind == "tubes":              # between two cover calls of opposite sizes; any size itself
                size = ("large", "small")[int(rng.integers(0, 2))]
            else:
                nth = seen.get(family, 0)
                if family in ("bg_sites", "bg_thal") and bg_size is not None:
                    size = "small" if bg_size == "large" else "large"
                elif nth == 0:
                    size = "large" if first_large else "small"
                elif nth == 1:
                    size = "small" if first_large else "large"
                else:
                    size = ("large", "small")[int(rng.integers(0, 2))]
            seen[family] = seen.get(family, 0) + (kind != "tubes")
            calls.append(Call(seed, len(calls), family, kind, size, name))
    # chains share inputs; k differs between the calls of a family where it has one; one chemistry and threshold in "chem"
    shared = {}
    for c in calls:
        c.shared = shared.setdefault(c.block if c.block != "single" else f"single{c.index}", {})
    ks = {f: list(rng.permutation(len(KS[f]))) for f in KS}
    ks["bg_thal"] = ks["bg_sites"]                 # one list: the chain's k and the other calls' differ
    chem_pick = (("ntthal", "primer3")[int(rng.integers(0, 2))], float((10.0, 25.0, 47.0)[int(rng.integers(0, 3))]))
    drawn = {}
    for c in calls:
        r = c.rng(1)
        if c.family in KS and not (c.block.startswith("background:") and "k" in c.shared):
            pick = KS[c.family][ks[c.family].pop(0) % len(KS[c.family])] if ks[c.family] else \
                KS[c.family][int(r.integers(0, len(KS[c.family])))]
            c.p["k"] = pick
            if c.block.startswith("background:"):
                c.shared["k"] = pick
        elif c.block.startswith("background:"):
            c.p["k"] = c.shared["k"]
        if c.block.startswith("chem:"):
            c.p["chem"], c.p["thr"] = chem_pick
        if c.kind == "tubes":                      # one split that can use several tubes, one at any limit
            c.p.update(T=int(r.choice([3, 64])), T2=int(r.choice([1, 3, 64])))
        PARAMS[c.kind](c, r)
        drawn[c.index] = bool(r.random() < 0.25)
    # the thal record, coverage, thinning and the site screen read none of the options: a draw that falls on one of them
    # passes to the next call of a family that reads some (and has no draw of its own), so none is spent on a no-op
    carry = 0
    for c in calls:
        names = OPTIONS_OF.get(c.family)
        if not names:
            carry += drawn[c.index]
            continue
        if drawn[c.index] or carry:
            carry -= not drawn[c.index]
            r = c.rng(5)
            name = names[int(r.integers(0, len(names)))]
            c.option = (name, OPTIONS[name][0])
    return calls


def neighbours(calls) -> set:
    """(kind, kind) of every two calls that follow each other."""
    return {(a.kind, b.kind) for a, b in zip(calls, calls[1:])}


# ---- parameters and inputs of every kind of call -----------------------------------------------------------------------

def p_any(c, r):
    if c.size == "large":
        n = int(r.integers(300, 401))
        if c.p["k"] == 20:                          # the oracle's 20-mer tables: 300..400 would take half a session's time
            n -= 60
        n += n % 24 == 0
    else:
        n = int(r.choice([63, 64, 65]))
    k = c.p["k"]
    c.p.update(n=n, skew=bool(r.integers(0, 4) == 0), planes=bool(r.integers(0, 3) > 0),
               dev=("planes", "edges")[int(r.integers(0, 2))])
    c.p.setdefault("chem", ("ntthal", "primer3", "ntthal37")[int(r.integers(0, 3))])
    c.p.setdefault("thr", float(r.choice([-2500.0, -5000.0] if k <= 9 else [-9000.0, -5000.0, -2500.0])))
    r0 = int(r.integers(0, n)); r1 = int(r.integers(r0 + 1, n + 1))
    c0 = int(r.integers(0, n)); c1 = int(r.integers(c0 + 1, n + 1))
    c.p["rect"] = (r0, r1, c0, c1)


def d_any(c):
    r, n, k = c.rng(2), c.p["n"], c.p["k"]
    prob = r.dirichlet([0.7] * 4) if c.p["skew"] else None
    pool = [s.tobytes().decode() for s in _ACGT[r.choice(4, size=(n, k), p=prob)]]
    for j in range(min(8, n // 4)):              # reverse-complement partners: conflicts at every threshold drawn
        pool[n // 2 + j] = rc(pool[j])
    return {"pool": pool}


def p_end(c, r):
    n = int(r.integers(200, 301)) if c.size == "large" else int(r.integers(40, 71))
    c.p.update(n=n, n_a=int(r.integers(1, n)), planes=True, dev=None)
    c.p.setdefault("chem", ("ntthal", "primer3")[int(r.integers(0, 2))])
    c.p.setdefault("thr", float(r.choice([10.0, 25.0, 47.0])))


def d_end(c):
    """Random oligos, partners that pair with another oligo's 3' end, self-complementary ones (even k), and pairs whose
    last DP row is empty (oligo 1 ends in A, the partner holds no T)."""
    r, n, k = c.rng(2), c.p["n"], c.p["k"]
    P = [rand_seq(r, k) for _ in range(n)]
    for j in range(min(12, n // 4)):
        tail = P[j][-min(k, max(2, (3 * k) // 4)):]
        P[n // 2 + j] = (rc(tail) + P[n // 2 + j])[:k]
    if k % 2 == 0:
        for j in range(4):
            h = rand_seq(r, k // 2)
            P[n // 4 + j] = h + rc(h)
    noT = lambda q: "".join("ACG"[x] for x in r.integers(0, 3, q))
    for j in range(3):
        P[n - 1 - 3 * j] = "C" + noT(k - 2) + "A"
        P[n - 2 - 3 * j] = noT(k - 1) + "G"
        P[n - 3 - 3 * j] = noT(k - 1) + "A"
    return {"pool": P}


def p_ab(c, r):
    lo, hi = (120, 201) if c.size == "large" else (20, 41)
    c.p.update(n_a=int(r.integers(lo, hi)), n_b=int(r.integers(lo, hi)), mixed=int(r.integers(12, 25)),
               chem=("ntthal", "primer3", "ntthal37")[int(r.integers(0, 3))], thr=float(r.choice([-9000.0, -6000.0])))


def d_ab(c):
    r, (k_a, k_b), n_a, n_b = c.rng(2), c.p["k"], c.p["n_a"], c.p["n_b"]
    A, B = [rand_seq(r, k_a) for _ in range(n_a)], [rand_seq(r, k_b) for _ in range(n_b)]
    for j in range(min(12, n_a, n_b)):            # B rows holding the reverse complement of (a part of) an A row
        a = A[j]
        if k_b <= k_a:
            at = int(r.integers(0, k_a - k_b + 1))
            B[j] = rc(a[at:at + k_b])
        else:
            at = int(r.integers(0, k_b - k_a + 1))
            B[j] = B[j][:at] + rc(a) + B[j][at + k_a:]
    q = c.p["mixed"]
    return {"A": A, "B": B, "mix": A[:q] + B[:q] + A[q:q + 3]}


def p_detail(c, r):
    c.p.update(n=int(r.integers(200, 301)) if c.size == "large" else int(r.integers(50, 81)),
               mode=("any", "end1")[int(r.integers(0, 2))], chem=("ntthal", "primer3")[int(r.integers(0, 2))])


def d_detail(c):
    r, n, k = c.rng(2), c.p["n"], c.p["k"]
    a, b = [rand_seq(r, k) for _ in range(n)], [rand_seq(r, k) for _ in range(n)]
    for j in range(0, n, 5):                       # every fifth pair holds a designed duplex with a bulge or a mismatch
        x = rc(a[j])
        if k >= 9:
            at = int(r.integers(2, k - 2))
            x = x[:at] + "ACGT"[("ACGT".index(x[at]) + 1) % 4] + x[at + 1:]
        b[j] = x
    return {"a": a, "b": b}


def alignment(r, rows, length, seg, stride) -> np.ndarray:
    """uint8 (rows, L): two clades off one ancestor, point mutations, '-' and 'N' runs; L leaves a partial segment."""
    L = int(length)
    if L >= seg and (L - seg) % stride == 0:
        L += int(r.integers(1, stride))
    anc = r.integers(0, 4, L)
    clade = anc.copy()
    mut = r.random(L) < 0.05
    clade[mut] = r.integers(0, 4, int(mut.sum()))
    out = np.empty((rows, L), dtype=np.uint8)
    for i in range(rows):
        row = (anc if i % 3 else clade).copy()
        mut = r.random(L) < float(r.choice([0.0, 0.01, 0.04]))
        row[mut] = r.integers(0, 4, int(mut.sum()))
        s = _ACGT[row].copy()
        for ch, longest in ((ord("-"), 30), (ord("N"), 10)):
            for _ in range(int(r.integers(1, 4))):
                at, ln = int(r.integers(0, L)), int(r.integers(1, longest + 1))
                s[at:at + ln] = ch
        out[i] = s
    return out


def p_align(c, r):
    seg, stride, W = WINDOWS[int(r.integers(0, 3))]
    if c.size == "large":
        rows, length = int(r.integers(24, 41)), int(r.integers(3000, 5001))
    else:
        rows, length = int(r.integers(8, 13)), int(r.integers(1200, 2001))
    if seg == 60:                                  # 30-column strides: many segments per row
        rows, length = max(8, rows // 2), max(1200, length // 2)
    c.p.update(rows=rows, length=length, seg=seg, stride=stride, W=W)


def p_stage_a(c, r):
    p_align(c, r)
    c.p.update(iters=int(r.integers(12, 41)), mms=int(r.integers(1, 3)), seeded=int(r.integers(0, 2)),
               n_seed=int(r.integers(1, 6)))


def d_align(c):
    r = c.rng(2)
    return {"g": alignment(r, c.p["rows"], c.p["length"], c.p["seg"], c.p["stride"])}


def window_primers(r, g, n, k, seg, stride, W, subs_max=2):
    """n forward and n reverse primers: half from head / tail windows of random segments (reverse ones reverse
    complemented), a quarter from anywhere, a quarter random; 0..subs_max substitutions."""
    rows, L = g.shape
    P = cm.n_partitions(L, seg, stride)
    out = ([], [])
    for d in (0, 1):
        while len(out[d]) < n:
            q = len(out[d]) % 4
            if q == 3 or P == 0:
                out[d].append(rand_seq(r, k))
                continue
            i = int(r.integers(0, rows))
            if q == 2:
                col = int(r.integers(0, L - k + 1))
            else:
                col = int(r.integers(0, P)) * stride + (seg - W if d else 0) + int(r.integers(0, W - k + 1))
            w = g[i, col:col + k].tobytes().decode()
            if set(w) - set("ACGT"):
                continue
            w = list(w)
            for at in r.choice(k, size=int(r.integers(0, subs_max + 1)), replace=False):
                w[at] = "ACGT"[("ACGT".index(w[at]) + int(r.integers(1, 4))) % 4]
            w = "".join(w)
            out[d].append(rc(w) if d else w)
    return out


def p_coverage(c, r):
    p_align(c, r)
    k = c.p["k"]
    hi = 121 if c.size == "large" else 31
    c.p.update(n_f=int(r.integers(10, hi)), n_r=int(r.integers(10, hi)), M=int(r.integers(0, 4)),
               E=int(r.choice([0, 1, 3, k])), form=("host", "packed")[int(r.integers(0, 2))])


def d_coverage(c):
    d = d_align(c)
    r, p = c.rng(3), c.p
    n = max(p["n_f"], p["n_r"])
    fwd, rev = window_primers(r, d["g"], n, p["k"], p["seg"], p["stride"], p["W"])
    d["fwd"], d["rev"] = fwd[:p["n_f"]], rev[:p["n_r"]]
    d["fwd"][-3:], d["rev"][-3:] = d["fwd"][:3], d["rev"][:3]
    return d


def p_thin(c, r):
    p_coverage(c, r)
    c.p.update(min_gain=int(r.integers(1, 3)), n_forced=int(r.integers(0, 4)),
               form=("host", "dev", "packed")[int(r.integers(0, 3))])


def d_thin(c):
    d = d_coverage(c)
    r, n = c.rng(4), c.p["n_f"] + c.p["n_r"]
    forced = np.zeros(n, dtype=np.uint8)
    forced[r.choice(n, size=c.p["n_forced"], replace=False)] = 1
    d["forced"] = forced if c.p["n_forced"] else None
    return d


def graph(r, n, skewed):
    """A directed conflict matrix: random pairs (skewed: a few hubs besides), a path over the first nodes (rounds of
    the cover), a clique of five (tubes), self loops (nodes no tube takes)."""
    b = np.triu(r.random((n, n)) < min(1.0, 3.0 / max(n, 1)), 1)
    if skewed and n > 8:
        hubs = r.choice(n, size=3, replace=False)
        b[hubs] |= r.random((3, n)) < 0.3
    idx = np.arange(min(n, 24))
    b[idx[:-1], idx[1:]] = True
    q = np.arange(min(n, 5)) + max(0, n - 5)
    b[np.ix_(q, q)] = True
    b[q, q] = False
    loops = np.arange(0, n, 17)
    b[loops, loops] = True
    return b


def p_graph(c, r):
    if c.size == "small":
        n = int(r.choice([1, 63, 64, 65]))
    else:                                          # every other large case at 200..300, where the host form screens too
        n = int(r.integers(200, 301)) if r.integers(0, 2) else int(r.integers(301, 1001))
    c.p.update(n=n, k=int(r.choice([13, 16, 20])), skewed=bool(r.integers(0, 2)), pad_garbage=bool(r.integers(0, 2)),
               host=n <= 300, chem="ntthal", thr=float(r.choice([-6000.0, -9000.0])))
    if c.p["host"] and n > 65:                     # the oracle screens this pool: 20-mers cost four times 13-mers
        c.p["k"] = int(r.choice([13, 16]))


def d_graph(c):
    r, n, k = c.rng(2), c.p["n"], c.p["k"]
    words = crm.random_words(n, k, r)
    if c.p["host"]:                                # the host form screens the pool: plant conflicts
        for j in range(min(6, n // 4)):
            w = rc(words[j])
            if w not in words:
                words[n // 2 + j] = w
    return {"words": words, "b": graph(r, n, c.p["skewed"])}


def stream_records(r, size, k):
    """Records of a background: random bases with a lower-case run, an N run and IUPAC codes; one record shorter than
    k always, and at the large end one longer than two runs of the kernel (2 x 2,048 columns)."""
    if size == "large":
        lens = [int(r.integers(4200, 6001))] + [int(r.integers(300, 1500)) for _ in range(int(r.integers(1, 3)))]
    else:
        lens = [int(r.integers(300, 900)) for _ in range(int(r.integers(1, 3)))]
    recs = []
    for ln in lens:
        s = bytearray(rand_seq(r, ln).encode())
        for fill, longest in ((b"n", 6), (b"N", 12), (b"R", 1), (b"a", 9)):
            at, q = int(r.integers(k, ln - k)), int(r.integers(1, longest + 1))
            s[at:at + q] = fill * q
        recs.append(s.decode())
    recs.insert(int(r.integers(0, len(recs) + 1)), rand_seq(r, int(r.integers(0, k))))
    return recs


def stream_primers(r, recs, n, k):
    """Primers of a background: windows of the records and reverse complements of windows with 0..2 substitutions,
    random words, the first k columns of the longest record (a site whose template has no left flank), and a forward /
    reverse pair that faces each other 60..260 columns apart (an amplicon when both sites are stable)."""
    long = max(recs, key=len)
    out = [long[:k]] if set(long[:k]) <= set("ACGT") else []
    for _ in range(50):
        a = int(r.integers(0, max(1, len(long) - 300)))
        b = a + int(r.integers(60, 261))
        f, w = long[a:a + k], long[b:b + k]
        if len(w) == k and set(f + w) <= set("ACGT"):
            out += [f, rc(w)]
            break
    while len(out) < n:
        q = len(out) % 5
        if q == 4:
            out.append(rand_seq(r, k))
            continue
        rec = recs[int(r.integers(0, len(recs)))]
        if len(rec) < k:
            continue
        at = int(r.integers(0, len(rec) - k + 1))
        w = rec[at:at + k]
        if set(w) - set("ACGT"):
            continue
        w = list(w)
        for x in r.choice(k, size=int(r.integers(0, 3)), replace=False):
            w[x] = "ACGT"[("ACGT".index(w[x]) + int(r.integers(1, 4))) % 4]
        w = "".join(w)
        out.append(rc(w) if q % 2 else w)
    return out[:n]


def p_bg(c, r):
    if c.block.startswith("background:") and "M" in c.shared:
        for key in ("n", "M", "E", "chem", "thr", "mode", "dseed"):
            c.p[key] = c.shared[key]
    else:
        k = c.p["k"]
        M = int(r.integers(0, 4))
        if k == 8:
            M = min(M, 1)                          # 8-mers within 2+ mismatches: sites by the ten thousand
        c.p.update(n=int(r.integers(40, 151)) if c.size == "large" else int(r.integers(10, 41)), M=M,
                   E=int(r.choice([0, 1, 3])), dseed=int(r.integers(1 << 30)))
        c.p.setdefault("chem", ("ntthal", "primer3")[int(r.integers(0, 2))])
        c.p.setdefault("thr", float(r.choice([10.0, 25.0, 47.0])))
        c.p["mode"] = "any" if c.kind == "thal_any" else ("any", "end1")[int(r.integers(0, 2))]
        if c.block.startswith("background:"):
            c.shared.update({key: c.p[key] for key in ("n", "M", "E", "chem", "thr", "mode", "dseed")})
    c.p["packed"] = bool(r.integers(0, 2))
    if c.kind in ("flank", "amplicons"):
        c.p["flank"] = int(r.integers(1, 5)) if c.kind == "flank" else int(r.integers(0, 5))
        c.p["flank"] = min(c.p["flank"], (32 - c.p["k"]) // 2)
    else:
        c.p["flank"] = 0
    if c.kind == "amplicons":
        c.p.update(min_len=int(r.integers(c.p["k"], 80)), max_len=int(r.integers(200, 601)))


def d_bg(c):
    if "records" not in c.shared:
        r = np.random.default_rng([c.p["dseed"], c.p["k"]])
        c.shared["records"] = stream_records(r, c.size, c.p["k"])
        c.shared["primers"] = stream_primers(r, c.shared["records"], c.p["n"], c.p["k"])
    return {"records": c.shared["records"], "primers": c.shared["primers"]}


PARAMS = {"any": p_any, "end": p_end, "ab": p_ab, "detail": p_detail, "stage_a": p_stage_a, "coverage": p_coverage,
          "thin": p_thin, "cover": p_graph, "tubes": p_graph, "sites": p_bg, "thal": p_bg, "thal_any": p_bg,
          "flank": p_bg, "flank0": p_bg, "amplicons": p_bg}
DATA = {"any": d_any, "end": d_end, "ab": d_ab, "detail": d_detail, "stage_a": d_align, "coverage": d_coverage,
        "thin": d_thin, "cover": d_graph, "tubes": d_graph, "sites": d_bg, "thal": d_bg, "thal_any": d_bg,
        "flank": d_bg, "flank0": d_bg, "amplicons": d_bg}


# ---- expected values ---------------------------------------------------------------------------------------------------

def fields(prefix, arr, names=None) -> dict:
    """A structured array as one plain array per field."""
    return {f"{prefix}.{f}": np.ascontiguousarray(arr[f]) for f in (names or arr.dtype.names)}


def pack_bits(cf) -> np.ndarray:
    """uint8 / bool (R, C) -> uint64 (R, ceil(C / 64)), bit j of row i = cf[i, j], padding clear."""
    R, Cc = cf.shape
    words = (Cc + 63) // 64
    full = np.zeros((R, words * 64), dtype=np.uint8)
    full[:, :Cc] = cf != 0
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(R, words)


def edge_dg(dg) -> np.ndarray:
    """What an edge of the host lists carries: the dG as Edge::get_dg() reads the "{:.2}" text of the %g value."""
    return np.array([o.round_fixed_f32(o.round_g_f32(float(x)), 2) for x in dg], dtype=np.float32)


def end_rule(tt, thr) -> np.ndarray:
    """od-msspe's SELF_END rule on a pair: conflict iff !(round_fixed_f32(max(0, t), 2) < float32(thr))."""
    thr32 = float(np.float32(thr))
    te = np.maximum(tt, 0.0)
    vals, inv = np.unique(te, return_inverse=True)
    hit = np.array([not o.round_fixed_f32(float(v), 2) < thr32 for v in vals], dtype=np.uint8)
    return hit[inv].reshape(te.shape)


def end_t(tt) -> np.ndarray:
    return np.array([o.round_fixed_f32(float(max(x, 0.0)), 2) for x in tt], dtype=np.float32)


def pair_block(A, B, mode, args):
    """(dG, t) over A x B of any two lengths, thal per pair: +inf / 0 where there is no structure."""
    dg, tt = np.empty((len(A), len(B))), np.empty((len(A), len(B)))
    T = tables()

    def row(i):
        for j, b in enumerate(B):
            res = o.thal(T, A[i], b, mode, args)
            dg[i, j] = np.inf if res.no_structure else res.dG
            tt[i, j] = 0.0 if res.no_structure else res.t

    with ThreadPoolExecutor(8) as ex:              # the oracle library releases the GIL and is re-entrant
        list(ex.map(row, range(len(A))))
    return dg, tt


def any_rule(dg, thr) -> np.ndarray:
    cf = np.zeros(dg.shape, dtype=np.uint8)
    for i, j in zip(*np.nonzero(dg < thr + 1000.0)):   # a conflict needs dG within rounding of the threshold
        cf[i, j] = o.edge_decision(float(dg[i, j]), thr)
    return cf


def square_want(dg, tt, cf, rect, dev, planes, value, rounded):
    """The outputs every square screen shares: host planes / bits / counts / sorted edges, and the device block."""
    r0, r1, c0, c1 = rect
    want = {"bits": cf, "rc": cf.sum(1).astype(np.uint32)}
    if planes:
        want.update(dg=dg, tm=tt)
    ii, jj = np.nonzero(cf)
    want.update({"edges.a": ii.astype(np.uint32), "edges.b": jj.astype(np.uint32), "edges.v": rounded(value[ii, jj])})
    sub = cf[r0:r1, c0:c1]
    rcw = np.full(cf.shape[0], RC_BASE, dtype=np.uint32)
    rcw[r0:r1] += sub.sum(1).astype(np.uint32)
    want["dev.rc"] = rcw
    if dev == "planes":
        want.update({"dev.bitmap": pack_bits(sub), "dev.dg": dg[r0:r1, c0:c1], "dev.tm": tt[r0:r1, c0:c1]})
    else:
        bi, bj = np.nonzero(sub)
        want.update({"dev.count": int(sub.sum()), "dev.edges.a": (bi + r0).astype(np.uint32),
                     "dev.edges.b": (bj + c0).astype(np.uint32), "dev.edges.v": value[r0:r1, c0:c1][bi, bj]})
    return want


def e_any(c):
    d, p = c.data(), c.p
    _, dg, cf, tt = o.pool_pairs(tables(), d["pool"], chem_args(p["chem"]), p["thr"], want_t=True)
    c.stats = {"conflicts": int(cf.sum()), "pairs": cf.size}
    return square_want(dg, tt, cf, p["rect"], p["dev"], p["planes"], dg, edge_dg)


def e_end(c):
    d, p = c.data(), c.p
    _, dg, _, tt = o.pool_pairs(tables(), d["pool"], chem_args(p["chem"]), 0.0, mode=o.END1, want_t=True)
    cf = end_rule(tt, p["thr"])
    c.stats = {"conflicts": int(cf.sum()), "pairs": cf.size}
    n_a = p["n_a"]
    want = square_want(dg, tt, cf, (0, n_a, n_a, p["n"]), "planes", True, tt, end_t)
    want = {key: v for key, v in want.items() if not key.startswith("dev.")}
    sub = cf[:n_a, n_a:]                            # rows A = pool[:n_a] against columns B = pool[n_a:]
    want.update({"ab.dg": dg[:n_a, n_a:], "ab.tm": tt[:n_a, n_a:], "ab.bits": sub, "ab.rc": sub.sum(1).astype(np.uint32)})
    return want


def e_ab(c):
    d, p = c.data(), c.p
    args = chem_args(p["chem"])
    dg, tt = pair_block(d["A"], d["B"], o.ANY, args)
    cf = any_rule(dg, p["thr"])
    c.stats = {"conflicts": int(cf.sum()), "pairs": cf.size}
    ii, jj = np.nonzero(cf)
    want = {"dg": dg, "tm": tt, "bits": cf, "rc": cf.sum(1).astype(np.uint32), "edges.a": ii.astype(np.uint32),
            "edges.b": jj.astype(np.uint32), "edges.v": edge_dg(dg[ii, jj])}
    mdg, _ = pair_block(d["mix"], d["mix"], o.ANY, args)
    mcf = any_rule(mdg, p["thr"])
    ii, jj = np.nonzero(mcf)
    want.update({"mixed.a": ii.astype(np.uint32), "mixed.b": jj.astype(np.uint32), "mixed.v": edge_dg(mdg[ii, jj])})
    return want


def e_detail(c):
    d, p = c.data(), c.p
    k, T, args = p["k"], tables(), chem_args(p["chem"])
    want = np.zeros(p["n"], dtype=THAL_DETAIL_DTYPE)
    mode = {"any": o.ANY, "end1": o.END1}[p["mode"]]
    for q, (x, y) in enumerate(zip(d["a"], d["b"])):
        r = o.thal(T, x, y, mode, args)
        if r.no_structure:
            want[q]["no_structure"] = r.no_structure   # a record without a structure is all zero but this
            continue
        want[q] = (r.dS, r.dH, r.dG, r.t, r.no_structure, r.n_pairs, 0, 0)
        want["ps1"][q, :k] = r.ps1[:k]
        want["ps2"][q, :k] = r.ps2[:k]
    c.stats = {"no_structure": int((want["no_structure"] != 0).sum())}
    return fields("rec", want)


def stage_a_seed(c, model, direction, plain):
    """Seed words of a seeded call: a shuffled prefix of the unseeded winners, a word of the index that did not win,
    one word absent from the index, one repeated."""
    r = c.rng(10 + direction)
    won = [w for w, _ in plain]
    seed = won[:min(c.p["n_seed"], max(len(won) - 1, 0))]
    rest = [w for w in model.vocab[::max(1, len(model.vocab) // 7)] if w not in won]
    seed += rest[:1] + ["ACGTTGCAAGCTTGCA"[:c.p["k"]]] + seed[:1]
    return [seed[i] for i in r.permutation(len(seed))]


def e_stage_a(c):
    d, p = c.data(), c.p
    seqs = [bytes(row).decode() for row in d["g"]]
    segs = o.Segments(seqs, p["seg"], p["stride"], p["W"], p["k"])
    want = {}
    d["seeds"] = {}
    for direction in (0, 1):
        plain = segs.candidates(direction, p["iters"], p["mms"])
        want[f"plain{direction}.words"] = [w for w, _ in plain]
        want[f"plain{direction}.freqs"] = np.array([f for _, f in plain], dtype=np.uint32)
        model = SeededModel(segs, direction)
        seed = stage_a_seed(c, model, direction, plain)
        d["seeds"][direction] = seed
        got = model.candidates(p["iters"], p["mms"], seed)
        want[f"seeded{direction}.words"] = [w for w, _ in got]
        want[f"seeded{direction}.freqs"] = np.array([f for _, f in got], dtype=np.uint32)
    c.stats = {"winners": len(want["plain0.words"]) + len(want["plain1.words"])}
    return want


def e_coverage(c):
    d, p = c.data(), c.p
    best, counts = cm.best_matrix(d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], p["M"], p["E"])
    exact, _ = cm.best_matrix(d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], 0, 0)
    c.stats = {"covered": int((best != 255).sum()), "segments": best.size}
    return {"best": best, "counts": counts, "exact": (exact == 0).astype(np.uint8)}


def e_thin(c):
    d, p = c.data(), c.p
    I = ptm.incidence(d["g"], p["seg"], p["stride"], p["W"], p["k"], d["fwd"], d["rev"], p["M"], p["E"])
    keep, order, gains, covered, c_all, c_kept, _rounds = ptm.greedy(I, p["min_gain"], d["forced"])
    n_seq = d["g"].shape[0]
    c.stats = {"kept": int(keep.sum()), "dropped": int((keep == 0).sum())}
    c.incidence = I
    return {"keep": keep, "order": order, "gains": gains, "covered": covered.astype(np.uint8).reshape(n_seq, -1),
            "covered_all": c_all, "covered_kept": c_kept}


def screen_graph(c):
    """The conflict matrix the host forms of cover / tubes screen for themselves."""
    d, p = c.data(), c.p
    _, _, cf, _ = o.pool_pairs(tables(), d["words"], chem_args(p["chem"]), p["thr"])
    return cf.astype(bool)


def e_cover(c):
    d, p = c.data(), c.p
    rank = crm.lex_rank(d["words"])
    deleted, rounds = crm.round_cover(crm.symmetrise(d["b"]), rank)
    want = {"dev.deleted": deleted.astype(np.uint8), "dev.n_deleted": int(deleted.sum()), "dev.rounds": rounds}
    c.stats = {"rounds": rounds}
    if p["host"]:
        deleted, rounds = crm.round_cover(crm.symmetrise(screen_graph(c)), rank)
        want.update({"host.deleted": deleted, "host.rounds": rounds})
    return want


def tubes_want(prefix, s, rank, T):
    tube, rounds = trm.rounds(s, rank, T)
    placed = tube[tube != trm.NONE]
    return {f"{prefix}.tube": tube, f"{prefix}.used": int(placed.max()) + 1 if placed.size else 0,
            f"{prefix}.unplaced": int((tube == trm.NONE).sum()), f"{prefix}.rounds": rounds}


def e_tubes(c):
    d, p = c.data(), c.p
    rank = crm.lex_rank(d["words"])
    want = tubes_want("dev", crm.symmetrise(d["b"]), rank, p["T"])
    want.update(tubes_want("dev2", crm.symmetrise(d["b"]), rank, p["T2"]))
    c.stats = {"used": want["dev.used"], "unplaced": want["dev.unplaced"]}
    if p["host"]:
        want.update(tubes_want("host", crm.symmetrise(screen_graph(c)), rank, p["T"]))
    return want


def e_sites(c):
    d, p = c.data(), c.p
    counts, sites = bgm.sites(d["records"], d["primers"], p["M"], p["E"])
    c.stats = {"sites": len(sites)}
    want = {"counts": counts, "starts": bgm.record_starts(d["records"])[0]}
    want.update(fields("sites", sites))
    return want


def scored(c, flank):
    """The scored sites of a background case at a flank; the calls of a chain share them."""
    d, p = c.data(), c.p
    key = ("scored", flank)
    if key not in c.shared:
        c.shared[key] = bfm.scored_sites(tables(), d["records"], d["primers"], p["M"], p["E"], p["mode"], p["thr"],
                                         chem_args(p["chem"]), flank)
    return c.shared[key]


def e_thal(c):
    d, p = c.data(), c.p
    counts, stable, recs = scored(c, p["flank"])
    _classes, truncated = bfm.class_stats(d["records"], d["primers"], recs, p["flank"]) if len(recs) else (0, 0)
    c.stats = {"sites": len(recs), "stable": int(stable.sum()), "truncated": truncated if p["flank"] else 0}
    want = {"counts": counts, "stable": stable, "starts": bgm.record_starts(d["records"])[0]}
    want.update(fields("sites", recs))
    return want


def e_amplicons(c):
    d, p = c.data(), c.p
    counts, stable, recs = scored(c, p["flank"])
    amp_counts, total, amps = bam.amplicons_of(len(d["primers"]), p["k"], recs, d["records"], p["min_len"], p["max_len"])
    c.stats = {"sites": len(recs), "stable": int(stable.sum()), "amplicons": total, "truncated": 0}
    want = {"counts": counts, "stable": stable, "amp_counts": amp_counts, "total": total,
            "starts": bgm.record_starts(d["records"])[0]}
    want.update(fields("amps", amps))
    return want


EXPECT = {"any": e_any, "end": e_end, "ab": e_ab, "detail": e_detail, "stage_a": e_stage_a, "coverage": e_coverage,
          "thin": e_thin, "cover": e_cover, "tubes": e_tubes, "sites": e_sites, "thal": e_thal, "thal_any": e_thal,
          "flank": e_thal, "flank0": e_thal, "amplicons": e_amplicons}


def expect(c: Call) -> dict:
    """The expected outputs of a call (computed once), and c.stats: what the non-triviality counters read."""
    if c._want is None:
        c.stats = {}
        c._want = EXPECT[c.kind](c)
    return c._want


def counters(calls) -> dict:
    """What keeps a session from being vacuous, from the expected values of its calls (expect() has run on each)."""
    st = lambda kinds, key: [c.stats.get(key, 0) for c in calls if c.kind in kinds]
    some = lambda kind: any(0 < c.stats["conflicts"] < c.stats["pairs"] for c in calls if c.kind == kind)
    bg = ("thal", "thal_any", "flank", "flank0", "amplicons")
    return {
        "any_some_conflicts": some("any"), "end_some_conflicts": some("end"),
        "background_sites": max(st(("sites",) + bg, "sites")), "background_stable": max(st(bg, "stable")),
        "background_truncated": max(st(bg, "truncated")), "amplicons": max(st(("amplicons",), "amplicons")),
        "thin_dropped": max(st(("thin",), "dropped")), "thin_kept": max(st(("thin",), "kept")),
        "tubes_used": max(st(("tubes",), "used")), "tubes_unplaced": max(st(("tubes",), "unplaced")),
        "cover_rounds": max(st(("cover",), "rounds")),
    }


# ---- running a call on an engine --------------------------------------------------------------------------------------

class Device:
    """Raw device buffers through the engine's own msspe_device_put / _get / _free (no torch): every output starts as a
    sentinel pattern, with GUARD elements more behind it that have to come back untouched."""

    def __init__(self, eng):
        self.eng, self.owned = eng, []

    def put(self, arr) -> int:
        a = np.ascontiguousarray(arr)
        dev = C.c_void_p()
        self.eng._check(self.eng.L.msspe_device_put(self.eng.ptr, a.ctypes.data, a.nbytes, C.byref(dev)))
        self.owned.append(int(dev.value))
        return int(dev.value)

    def get(self, ptr, count, dtype) -> np.ndarray:
        return self.eng.device_get(ptr, count * np.dtype(dtype).itemsize).view(dtype)

    def close(self):
        for ptr in self.owned:
            self.eng.device_free(ptr)
        self.owned = []


def sentinel(count, dtype):
    return np.full((count + GUARD) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype)


def guard_ok(buf, count, what, problems):
    """Everything behind the first `count` elements of a fetched buffer is still the sentinel."""
    if not (np.ascontiguousarray(buf[count:]).view(np.uint8) == FILL).all():
        problems.append(f"{what}: bytes behind the defined extent were written")


def bits(bitmap, ncols):
    return np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), axis=1, bitorder="little")[:, :ncols]


def sorted_edges(rec, prefix):
    rec = rec[np.lexsort((rec["b"], rec["a"]))]
    return {f"{prefix}.a": rec["a"].copy(), f"{prefix}.b": rec["b"].copy(), f"{prefix}.v": rec["v"].copy()}


EDGE_DEV = np.dtype([("a", np.uint32), ("b", np.uint32), ("v", np.float64)])


def r_square(c, m, dv, host, host_edges, dev_call, dev_edges_call, k, want):
    """Host screen, host edge list, and one device block on dirty buffers (planes or edges) of a square screen."""
    p, d = c.p, c.data()
    chem = chem_obj(m, p["chem"])
    problems, got = [], {}
    out = host(d["pool"], chem, p["thr"], want_dg=p["planes"], want_tm=p["planes"])
    n = len(d["pool"])
    got.update(bits=bits(out["bitmap"], n), rc=out["row_conflicts"])
    if p["planes"]:
        got.update(dg=out["dg"], tm=out["tm"])
    edges, count = host_edges(d["pool"], chem, p["thr"], capacity=len(want["edges.a"]) + 8)
    vname = edges.dtype.names[2]
    got.update({"edges.a": edges["a"].copy(), "edges.b": edges["b"].copy(), "edges.v": edges[vname].copy()})
    if dev_call is None:
        return got, problems
    r0, r1, c0, c1 = p["rect"]
    R, Cc = r1 - r0, c1 - c0
    words = (Cc + 63) // 64
    d_pool = dv.put(m.pack_oligos(d["pool"]))
    d_rc = dv.put(np.full(n, RC_BASE, dtype=np.uint32))
    if p["dev"] == "planes":
        d_bm, d_dg, d_tm = dv.put(sentinel(R * words, np.uint64)), dv.put(sentinel(R * Cc, np.float64)), \
            dv.put(sentinel(R * Cc, np.float64))
        dev_call(d_pool, n, k, chem, p["thr"], (r0, r1), (c0, c1), d_rc, d_bm, d_dg, d_tm)
        bm = dv.get(d_bm, R * words + GUARD, np.uint64)
        dg, tm = dv.get(d_dg, R * Cc + GUARD, np.float64), dv.get(d_tm, R * Cc + GUARD, np.float64)
        for buf, cnt, what in ((bm, R * words, "bitmap"), (dg, R * Cc, "dG plane"), (tm, R * Cc, "t plane")):
            guard_ok(buf, cnt, what, problems)
        got.update({"dev.bitmap": bm[:R * words].reshape(R, words), "dev.dg": dg[:R * Cc].reshape(R, Cc),
                    "dev.tm": tm[:R * Cc].reshape(R, Cc)})
    else:
        cap = want["dev.count"] + 8
        d_e, d_cnt = dv.put(sentinel(cap, EDGE_DEV)), dv.put(np.zeros(1, dtype=np.uint64))
        dev_edges_call(d_pool, n, k, chem, p["thr"], (r0, r1), (c0, c1), d_e, cap, d_cnt, d_rc)
        cnt = int(dv.get(d_cnt, 1, np.uint64)[0])
        rec = dv.get(d_e, cap + GUARD, EDGE_DEV)
        guard_ok(rec, min(cnt, cap), "edge list", problems)
        got["dev.count"] = cnt
        got.update(sorted_edges(rec[:min(cnt, cap)], "dev.edges"))
    got["dev.rc"] = dv.get(d_rc, n, np.uint32)
    return got, problems


def r_any(c, eng, m, dv, want):
    return r_square(c, m, dv, eng.cross_dimer, eng.cross_dimer_edges, eng.cross_dimer_dev, eng.cross_dimer_edges_dev,
                    c.p["k"], want)


def r_end(c, eng, m, dv, want):
    p, d = c.p, c.data()
    got, problems = r_square(c, m, dv, eng.cross_dimer_end, eng.cross_dimer_end_edges, None, None, p["k"], want)
    n_a = p["n_a"]
    out = eng.cross_dimer_end_ab(d["pool"][:n_a], d["pool"][n_a:], chem_obj(m, p["chem"]), p["thr"])
    got.update({"ab.dg": out["dg"], "ab.tm": out["tm"], "ab.bits": bits(out["bitmap"], p["n"] - n_a),
                "ab.rc": out["row_conflicts"]})
    return got, problems


def r_ab(c, eng, m, dv, want):
    p, d = c.p, c.data()
    chem = chem_obj(m, p["chem"])
    out = eng.cross_dimer_ab(d["A"], d["B"], chem, p["thr"], want_dg=True, want_tm=True)
    got = {"dg": out["dg"], "tm": out["tm"], "bits": bits(out["bitmap"], len(d["B"])), "rc": out["row_conflicts"]}
    e, _ = eng.cross_dimer_ab_edges(d["A"], d["B"], chem, p["thr"], capacity=len(want["edges.a"]) + 8)
    got.update({"edges.a": e["a"].copy(), "edges.b": e["b"].copy(), "edges.v": e["dg"].copy()})
    e, _ = eng.cross_dimer_edges_mixed(d["mix"], chem, p["thr"], capacity=len(want["mixed.a"]) + 8)
    got.update({"mixed.a": e["a"].copy(), "mixed.b": e["b"].copy(), "mixed.v": e["dg"].copy()})
    return got, []


def r_detail(c, eng, m, dv, want):
    p, d = c.p, c.data()
    rec = eng.thal_detail(d["a"], d["b"], chem_obj(m, p["chem"]), p["mode"])
    return fields("rec", rec, THAL_DETAIL_DTYPE.names), []


def r_stage_a(c, eng, m, dv, want):
    p, d = c.p, c.data()
    g = d["g"]
    opt = m.KmerOpt(p["seg"], p["stride"], p["W"], p["k"], p["iters"], p["mms"])
    got = {}
    for direction in (0, 1):
        w, f = eng.kmer_candidates(g, opt, direction)
        got[f"plain{direction}.words"], got[f"plain{direction}.freqs"] = w, f
    handle = eng.put_rows_packed(g)
    try:
        if p["seeded"]:                             # both directions of the packed alignment at once
            both = eng.kmer_candidates_both_packed(handle, g.shape[0], g.shape[1], opt, seed_fwd=d["seeds"][0],
                                                   seed_rev=d["seeds"][1])
        else:                                       # one seeded call per direction: host rows, then packed
            both = (eng.kmer_candidates(g, opt, 0, seed=d["seeds"][0]),
                    eng.kmer_candidates_packed(handle, g.shape[0], g.shape[1], opt, 1, seed=d["seeds"][1]))
    finally:
        eng.device_free(handle)
    for direction in (0, 1):
        got[f"seeded{direction}.words"], got[f"seeded{direction}.freqs"] = both[direction]
    return got, []


def r_coverage(c, eng, m, dv, want):
    p, d = c.p, c.data()
    g = d["g"]
    opt = m.KmerOpt(p["seg"], p["stride"], p["W"], p["k"], 0, 0)
    got = {"exact": eng.segment_coverage(g, opt, d["fwd"], d["rev"])}
    if p["form"] == "host":
        got["best"], got["counts"] = eng.segment_coverage_mm(g, opt, d["fwd"], d["rev"], p["M"], p["E"], per_primer=True)
    else:
        handle = eng.put_rows_packed(g)
        try:
            got["best"], got["counts"] = eng.segment_coverage_mm_packed(handle, g.shape[0], g.shape[1], opt, d["fwd"],
                                                                        d["rev"], p["M"], p["E"], per_primer=True)
        finally:
            eng.device_free(handle)
    return got, []


def r_thin(c, eng, m, dv, want):
    p, d = c.p, c.data()
    opt = m.KmerOpt(p["seg"], p["stride"], p["W"], p["k"], 0, 0)
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin(d["g"], opt, d["fwd"], d["rev"], p["M"], p["E"],
                                                               p["min_gain"], d["forced"], p["form"])
    return {"keep": keep, "order": order, "gains": gains, "covered": covered, "covered_all": c_all,
            "covered_kept": c_kept}, []


def graph_words(b, pad_garbage):
    bm = pack_bits(b)
    n = b.shape[0]
    if pad_garbage and n % 64:                      # bits beyond n are not the call's to read
        bm[:, -1] |= ~np.uint64(0) << np.uint64(n % 64)
    return bm


def r_cover(c, eng, m, dv, want):
    p, d = c.p, c.data()
    n, k, problems, got = p["n"], p["k"], [], {}
    if p["host"]:
        got["host.deleted"] = eng.conflict_cover(d["words"], chem_obj(m, p["chem"]), p["thr"])
        got["host.rounds"] = eng.info("cover_rounds")
    d_pool, d_bm = dv.put(m.pack_oligos(d["words"])), dv.put(graph_words(d["b"], p["pad_garbage"]))
    d_del = dv.put(sentinel(n, np.uint8))
    got["dev.n_deleted"] = eng.conflict_cover_dev(d_pool, n, k, d_bm, d_del)
    got["dev.rounds"] = eng.info("cover_rounds")
    out = dv.get(d_del, n + GUARD, np.uint8)
    guard_ok(out, n, "deleted flags", problems)
    got["dev.deleted"] = out[:n]
    return got, problems


def r_tubes(c, eng, m, dv, want):
    p, d = c.p, c.data()
    n, k, problems, got = p["n"], p["k"], [], {}
    if p["host"]:
        tube, used, unplaced = eng.conflict_tubes(d["words"], chem_obj(m, p["chem"]), p["thr"], p["T"])
        got.update({"host.tube": tube, "host.used": used, "host.unplaced": unplaced,
                    "host.rounds": eng.info("tube_rounds")})
    d_pool, d_bm = dv.put(m.pack_oligos(d["words"])), dv.put(graph_words(d["b"], p["pad_garbage"]))
    for prefix, T in (("dev", p["T"]), ("dev2", p["T2"])):
        d_tube = dv.put(sentinel(n, np.uint8))
        got[f"{prefix}.used"], got[f"{prefix}.unplaced"] = eng.conflict_tubes_dev(d_pool, n, k, d_bm, d_tube, T)
        got[f"{prefix}.rounds"] = eng.info("tube_rounds")
        out = dv.get(d_tube, n + GUARD, np.uint8)
        guard_ok(out, n, "tube array", problems)
        got[f"{prefix}.tube"] = out[:n]
    return got, problems


def sort_records(rec, keys):
    return rec[np.lexsort(tuple(rec[key] for key in keys[::-1]))]


def r_sites(c, eng, m, dv, want):
    p, d = c.p, c.data()
    n_sites, problems = len(want["sites.pos"]), []
    if not p["packed"]:
        counts, starts, sites = eng.background_sites(d["records"], d["primers"], p["M"], p["E"], k=p["k"],
                                                     capacity=n_sites + 8)
    else:
        handle, total, starts = eng.put_stream_packed(d["records"])
        try:
            cap = n_sites + 8
            d_sites, d_count = dv.put(sentinel(cap, bgm.SITE_DTYPE)), dv.put(np.zeros(1, dtype=np.uint64))
            counts = eng.background_sites_packed(handle, total, d["primers"], p["M"], p["E"], k=p["k"],
                                                 d_sites=d_sites, capacity=cap, d_count=d_count)
            cnt = int(dv.get(d_count, 1, np.uint64)[0])
            raw = dv.get(d_sites, cap + GUARD, bgm.SITE_DTYPE)
        finally:
            eng.device_free(handle)
        guard_ok(raw, min(cnt, cap), "site list", problems)
        if cnt != n_sites:
            problems.append(f"site list: count {cnt}, expected {n_sites}")
        sites = sort_records(raw[:min(cnt, cap)], ("primer", "strand", "pos"))
    got = {"counts": counts, "starts": starts}
    got.update(fields("sites", sites, bgm.SITE_DTYPE.names))
    return got, problems


def r_thal(c, eng, m, dv, want):
    p, d = c.p, c.data()
    n_sites, problems = len(want["sites.pos"]), []
    chem = chem_obj(m, p["chem"])
    if not p["packed"]:
        counts, stable, starts, sites = eng.background_thal(d["records"], d["primers"], p["M"], p["E"], chem, p["thr"],
                                                            p["mode"], k=p["k"], capacity=n_sites + 8, flank=p["flank"])
    else:
        handle, total, starts = eng.put_stream_packed(d["records"])
        try:
            cap = n_sites + 8
            d_sites, d_count = dv.put(sentinel(cap, btm.SCORED_SITE_DTYPE)), dv.put(np.zeros(1, dtype=np.uint64))
            counts, stable = eng.background_thal_packed(handle, total, d["primers"], p["M"], p["E"], chem, p["thr"],
                                                        p["mode"], k=p["k"], d_sites=d_sites, capacity=cap,
                                                        d_count=d_count, flank=p["flank"])
            cnt = int(dv.get(d_count, 1, np.uint64)[0])
            raw = dv.get(d_sites, cap + GUARD, btm.SCORED_SITE_DTYPE)
        finally:
            eng.device_free(handle)
        guard_ok(raw, min(cnt, cap), "scored site list", problems)
        if cnt != n_sites:
            problems.append(f"scored site list: count {cnt}, expected {n_sites}")
        sites = sort_records(raw[:min(cnt, cap)], ("primer", "strand", "pos"))
    got = {"counts": counts, "stable": stable, "starts": starts}
    got.update(fields("sites", sites, btm.SCORED_SITE_DTYPE.names))
    return got, problems


def r_amplicons(c, eng, m, dv, want):
    p, d = c.p, c.data()
    n_amps, problems = len(want["amps.pos"]), []
    chem = chem_obj(m, p["chem"])
    if not p["packed"]:
        counts, stable, amp_counts, total, starts, lst = eng.background_amplicons(
            d["records"], d["primers"], p["M"], p["E"], chem, p["thr"], p["mode"], p["min_len"], p["max_len"], k=p["k"],
            capacity=n_amps + 8, flank=p["flank"])
    else:
        handle, total_len, starts = eng.put_stream_packed(d["records"])
        try:
            cap = n_amps + 8
            d_amps, d_count = dv.put(sentinel(cap, bam.AMPLICON_DTYPE)), dv.put(np.zeros(1, dtype=np.uint64))
            counts, stable, amp_counts, total = eng.background_amplicons_packed(
                handle, total_len, d["primers"], p["M"], p["E"], chem, p["thr"], p["mode"], p["min_len"], p["max_len"],
                record_start=starts, k=p["k"], d_amplicons=d_amps, capacity=cap, d_count=d_count, flank=p["flank"])
            cnt = int(dv.get(d_count, 1, np.uint64)[0])
            raw = dv.get(d_amps, cap + GUARD, bam.AMPLICON_DTYPE)
        finally:
            eng.device_free(handle)
        guard_ok(raw, min(cnt, cap), "amplicon list", problems)
        if cnt != n_amps:
            problems.append(f"amplicon list: count {cnt}, expected {n_amps}")
        lst = sort_records(raw[:min(cnt, cap)], ("pos", "len", "fwd", "rev"))
    got = {"counts": counts, "stable": stable, "amp_counts": amp_counts, "total": total, "starts": starts}
    got.update(fields("amps", lst, bam.AMPLICON_DTYPE.names))
    return got, problems


RUN = {"any": r_any, "end": r_end, "ab": r_ab, "detail": r_detail, "stage_a": r_stage_a, "coverage": r_coverage,
       "thin": r_thin, "cover": r_cover, "tubes": r_tubes, "sites": r_sites, "thal": r_thal, "thal_any": r_thal,
       "flank": r_thal, "flank0": r_thal, "amplicons": r_amplicons}


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
                eng.set_option(c.option[0], OPTIONS[c.option[0]][1])
        finally:
            dv.close()


def same(a, b) -> bool:
    if isinstance(b, list) or isinstance(a, list):
        return list(a) == list(b)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f"))


def differences(got: dict, want: dict) -> list[str]:
    """Names of the outputs that are not exactly the expected ones (and of those the call did not return)."""
    out = []
    for key, w in want.items():
        if key not in got:
            out.append(f"{key}: not returned")
        elif not same(got[key], w):
            g, w = np.asarray(got[key]), np.asarray(w)
            where = ""
            if g.shape == w.shape and g.size and g.dtype.kind in "biuf":
                bad = np.flatnonzero((g != w).reshape(-1))
                where = f", {bad.size} of {g.size} differ, first at {int(bad[0])}: got {g.reshape(-1)[bad[0]]!r} " \
                        f"expected {w.reshape(-1)[bad[0]]!r}" if bad.size else ""
            out.append(f"{key}: shape {g.shape} against {w.shape}{where}")
    return out


def image(got: dict) -> bytes:
    """The outputs of a call as bytes (the replay has to return the same ones)."""
    parts = []
    for key in sorted(got):
        v = got[key]
        parts.append(key.encode())
        parts.append(repr(v).encode() if isinstance(v, (list, int)) else np.ascontiguousarray(v).tobytes())
    return b"\0".join(parts)


def run_session(seed: int, eng, m, only: int | None = None, log=print) -> list[str]:
    """A whole session on one engine: every call against its expected value, the sentinels, and the replay of the first
    three calls.  only: run the schedule up to and including that call and check that call alone.  Returns the failures,
    each naming family, parameters, seed and call index."""
    calls = schedule(seed)
    failures, first = [], {}
    last = len(calls) - 1 if only is None else only
    for c in calls[:last + 1]:
        t0 = time.perf_counter()
        want = expect(c)
        t1 = time.perf_counter()
        got, problems = run_call(c, eng, m, want)
        t2 = time.perf_counter()
        if c.index < 3:
            first[c.index] = image(got)
        bad = [] if only is not None and c.index != only else differences(got, want) + problems
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
    """What a schedule exercises, as a set of items: families, k of every family, options, chain orders, window
    geometries, tube limits, entry forms.  The committed seeds together have to hold every item of required()."""
    out = set()
    for c in calls:
        out.add(("family", c.family))
        out.add(("kind", c.kind, c.size))
        if c.family in KS:
            out.add(("k", c.family, c.p["k"]))
        if c.option:
            out.add(("option", c.option[0]))
        if c.block != "single":
            out.add(("chain", c.block))
        if "seg" in c.p:
            out.add(("window", c.p["seg"]))
        if c.kind == "tubes":
            out |= {("T", c.p["T"]), ("T", c.p["T2"])}
        if c.kind in ("thal", "thal_any", "flank", "flank0", "amplicons"):
            out.add(("mode", c.p["mode"]))
            out.add(("chem", c.p["chem"]))
            out.add(("flank", c.p["flank"]))
    return out


def required() -> set:
    out = {("family", f) for f in FAMILIES} | {("option", x) for x in OPTIONS}
    out |= {("k", f, k) for f in KS for k in KS[f]}
    out |= {("chain", f"{name}:{d}") for name in ("background", "chem") for d in ("fwd", "rev")}
    out |= {("window", w[0]) for w in WINDOWS} | {("T", t) for t in (1, 3, 64)}
    out |= {("mode", x) for x in ("any", "end1")} | {("chem", x) for x in ("ntthal", "primer3")}
    out |= {("flank", f) for f in range(5)}
    return out
