"""Shared test helpers (pure Python, small inputs only)."""
from __future__ import annotations


def draw_dimer(oligo1: str, oligo2: str, ps1, ps2) -> list[str]:
    """ntthal's four alignment rows for a duplex (Primer3 2.6.1 thal.c drawDimer, restated).

    ps1[i-1] = partner in the REVERSED oligo 2 (0 = unpaired), ps2 likewise.  Rows are returned
    with ntthal's "SEQ\\t"/"STR\\t" prefixes; the reference's transcript
    (od-msspe/src/delta_g.rs:206-230) shows them tab-expanded.
    """
    o2 = oligo2[::-1]
    len1, len2 = len(oligo1), len(o2)
    d = ["", "", "", ""]
    n1 = 0
    while n1 < len1 and ps1[n1] == 0:
        n1 += 1
    n2 = 0
    while n2 < len2 and ps2[n2] == 0:
        n2 += 1
    if n1 >= n2:
        d[0] += oligo1[:n1]
        d[1] += " " * n1
        d[2] += " " * n1
        d[3] += " " * (n1 - n2) + o2[:n2]
    else:
        d[3] += o2[:n2]
        d[1] += " " * n2
        d[2] += " " * n2
        d[0] += " " * (n2 - n1) + oligo1[:n1]
    i, j = n1 + 1, n2 + 1
    while i <= len1:
        while i <= len1 and ps1[i - 1] != 0 and j <= len2 and ps2[j - 1] != 0:
            d[0] += " "
            d[1] += oligo1[i - 1]
            d[2] += o2[j - 1]
            d[3] += " "
            i += 1
            j += 1
        s1 = 0
        while i <= len1 and ps1[i - 1] == 0:
            d[0] += oligo1[i - 1]
            d[1] += " "
            s1 += 1
            i += 1
        s2 = 0
        while j <= len2 and ps2[j - 1] == 0:
            d[2] += " "
            d[3] += o2[j - 1]
            s2 += 1
            j += 1
        if s1 < s2:
            d[0] += "-" * (s2 - s1)
            d[1] += " " * (s2 - s1)
        elif s1 > s2:
            d[2] += " " * (s1 - s2)
            d[3] += "-" * (s1 - s2)
    return ["SEQ\t" + d[0], "SEQ\t" + d[1], "STR\t" + d[2], "STR\t" + d[3]]


def window_with_kmers(kmers: list[str], width: int) -> str:
    """A search window whose valid k-mers are exactly `kmers` in order: consecutive overlapping
    k-mers are merged, others are separated by '-' (which invalidates every k-mer covering it,
    od-msspe/src/main.rs:167)."""
    out = ""
    for km in kmers:
        if out and out[-(len(km) - 1):] == km[:-1]:
            out += km[-1]
        else:
            out += ("-" if out else "") + km
    assert len(out) <= width, (out, width)
    return out + "-" * (width - len(out))


_COMP = str.maketrans("ACGT", "TGCA")


def reverse_complement(s: str) -> str:
    return s.translate(_COMP)[::-1]


def stem_loop(rng, k: int) -> str:
    """A designed hairpin of length k: a stem of 4..7 pairs (shortened to fit) around a loop of 3..6 bases, at a
    random offset between random flanks.  Oligos shorter than the loop get no stem."""
    stem = int(rng.integers(4, 8))
    loop = int(rng.integers(3, 7))
    if 2 * stem + loop > k:
        stem = (k - loop) // 2
    if stem < 0:
        stem, loop = 0, k
    left = "".join("ACGT"[x] for x in rng.integers(0, 4, stem))
    mid = "".join("ACGT"[x] for x in rng.integers(0, 4, loop))
    core = left + mid + reverse_complement(left)
    pad = k - len(core)
    off = int(rng.integers(0, pad + 1))
    flank = "".join("ACGT"[x] for x in rng.integers(0, 4, pad))
    return flank[:off] + core + flank[off:]


def with_stem_loops(pool: list[str], k: int, rng, every: int = 4) -> list[str]:
    """Replaces every `every`-th oligo of the pool (in place) with a designed stem-loop; returns the pool."""
    for q in range(len(pool) // every):
        pool[every * q] = stem_loop(rng, k)
    return pool


def stage_b_pool(k: int, seed: int, n_random: int = 48, n_stem_loops: int = 32) -> list[str]:
    """Oligos of length k for the per-oligo statistics: random ones, designed stem-loops, palindromes (even k:
    self-complementary; odd k: a base between the halves), homopolymers, and the END1 corners (no partner for the
    3' base anywhere, with and without other pairs; a 3' base whose only partner is the 5' base)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    pool = [rand(k) for _ in range(n_random)]
    pool += [stem_loop(rng, k) for _ in range(n_stem_loops)]
    for _ in range(6):
        half = rand(k // 2)
        pool.append(half + rand(k % 2) + reverse_complement(half))
    pool += [("GC" * k)[:k], ("AT" * k)[:k], ("GGCC" * k)[:k]]
    pool += [b * k for b in "ACGT"]
    pool += ["A" * (k - 1) + "C", "G" * (k - 2) + "CA", "T" * (k - 1) + "A", "T" + "A" * (k - 1),
             ("CA" * k)[:k - 1] + "G"]
    assert all(len(s) == k for s in pool)
    return pool


# Chemistries of the stage-B parity tests (msspe_chem / pyoracle.p3_args keywords) and the statistics each one is
# there to move away from Primer3's defaults.  Every one keeps oligotm's salt term finite.
STAGE_B_CHEMS = {
    "primer3": ({}, ()),
    "ntthal": (dict(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0), ("tm", "self_any_th", "hairpin_th")),
    "dv0_dntp": (dict(dv=0.0, dntp=0.6), ("tm",)),
    "dv_below_dntp": (dict(dv=0.3, dntp=0.6), ("tm",)),
    "dv0_negative_dntp": (dict(dv=0.0, dntp=-0.5), ("tm",)),     # valid: oligotm zeroes dntp when dv == 0
    "mv1000_dv0": (dict(mv=1000.0, dv=0.0), ("tm", "self_any_th", "hairpin_th")),
    "mv10": (dict(mv=10.0), ("tm", "self_any_th", "hairpin_th")),
    "dna5": (dict(dna_conc=5.0), ("tm", "self_any_th")),
    "dna5000": (dict(dna_conc=5000.0), ("tm", "self_any_th")),
    "temp10": (dict(temp_c=10.0), ("hairpin_th",)),
    "temp60": (dict(temp_c=60.0), ("hairpin_th",)),
    "loop0": (dict(max_loop=0), ("self_any_th", "hairpin_th")),
    "loop3": (dict(max_loop=3), ("self_any_th", "hairpin_th")),
    "loop7": (dict(max_loop=7), ("self_any_th",)),
    "loop20": (dict(max_loop=20), ()),          # below 2k - 4 for 13-mers: self-dimers leave the one-lane route
}
# Lengths every chemistry meets (k <= 14: register tables; 15..32: split tables / one wave per oligo; 31-32), and
# all lengths, which a few chemistries meet.
STAGE_B_FAMILY_KS = (4, 13, 20, 32)
STAGE_B_ALL_KS = (2, 3, 4, 5, 7, 8, 10, 12, 13, 14, 16, 20, 24, 31, 32)
STAGE_B_ALL_KS_CHEMS = ("primer3", "ntthal", "loop3", "temp60")


def stage_b_cases():
    """(chemistry name, k) of the stage-B parity matrix; the pool of a case is stage_b_pool(k, 1000 + k)."""
    cases = [(c, k) for c in STAGE_B_CHEMS for k in STAGE_B_FAMILY_KS]
    cases += [(c, k) for c in STAGE_B_ALL_KS_CHEMS for k in STAGE_B_ALL_KS if k not in STAGE_B_FAMILY_KS]
    return cases
