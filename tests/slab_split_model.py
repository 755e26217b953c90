"""A Python model of csrc/slab_split.hpp: how a thal-scored site pass cuts a slab -- outer range [o0, o1) (runs, or
segment groups) against primers [p0, p1) -- whose count of matches overran a work list of cap entries.  Written from
the rule: aim at parts that come out half full (ceil(2 count / cap) of them, never more than the axis has elements),
cut the outer axis evenly while it has several elements, otherwise the primers; one element against one primer cannot
be cut.  A part is (o0, o1, p0, p1), the columns of msspe_host_slab_split."""


def cuts(lo: int, extent: int, parts: int) -> list:
    bounds = [lo + extent * q // parts for q in range(parts + 1)]
    return list(zip(bounds, bounds[1:]))


def slab_split_model(o0: int, o1: int, p0: int, p1: int, count: int, cap: int) -> list:
    want = -(-2 * count // cap)
    if o1 - o0 > 1:
        return [(a, b, p0, p1) for a, b in cuts(o0, o1 - o0, min(o1 - o0, want))]
    if p1 - p0 > 1:
        return [(o0, o1, a, b) for a, b in cuts(p0, p1 - p0, min(p1 - p0, want))]
    return []
