"""Nearest-neighbour tables other than the shipped ones (test infrastructure, no GPU): read and write a parameter
bundle or a Primer3 directory, and the variants the route tests use.  Every variant is a pure function of the stock
bundle; EXPECTED_ROUTES says which kernels the engine may use under it (msspe_host_table_routes, in the order of
msspe_amd.capi.TABLE_ROUTE_KEYS without "split_ok"), at ntthal's and at Primer3's default chemistry alike."""
from __future__ import annotations

from pathlib import Path

SECTIONS = ("stack.ds", "stack.dh", "stackmm.ds", "stackmm.dh", "tstack_tm_inf.ds", "tstack.dh", "tstack2.ds",
            "tstack2.dh", "dangle.ds", "dangle.dh", "loops.ds", "loops.dh", "triloop.ds", "triloop.dh",
            "tetraloop.ds", "tetraloop.dh")
BONUS_SECTIONS = ("triloop.ds", "triloop.dh", "tetraloop.ds", "tetraloop.dh")


def _read_bundle(path):
    """{section: [lines]} of a parameter bundle ('@ name count' headers)."""
    sections, name = {}, None
    for line in Path(path).read_text().splitlines():
        if line.startswith("#") or not line.strip():
            continue
        if line.startswith("@"):
            name = line.split()[1]
            sections[name] = []
        else:
            sections[name].append(line)
    return sections


def _perturbed(sections, step_s, step_h):
    """Shift every available entry of the stack / mismatch / terminal-stack / dangle entropies by
    a multiple of step_s and the stack enthalpies by a multiple of step_h (tables stay plausible:
    the point is that the engine computes with whatever the files hold)."""
    out = {}
    for name, lines in sections.items():
        step = {"stack.ds": step_s, "stackmm.ds": step_s, "tstack2.ds": step_s, "tstack_tm_inf.ds": step_s,
                "dangle.ds": step_s, "stack.dh": step_h}.get(name)
        if step is None:
            out[name] = list(lines)
            continue
        q, new = 0, []
        for line in lines:
            toks = []
            for t in line.split():
                if t != "inf":
                    q += 1
                    t = repr(round(float(t) + step * (q % 3 - 1), 6))
                toks.append(t)
            new.append(" ".join(toks))
        out[name] = new
    return out


def bundle_text(sections) -> str:
    return "# test bundle\n" + "".join(
        f"@ {name} {sum(len(l.split()) for l in lines)}\n" + "\n".join(lines) + "\n"
        for name, lines in sections.items())


def write_bundle(sections, path) -> Path:
    """One file with '@ name count' headers, as the engine ships its tables."""
    path = Path(path)
    path.write_text(bundle_text(sections))
    return path


def write_directory(sections, path) -> Path:
    """Primer3's 16 files, what ntthal reads with -path."""
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    assert sorted(sections) == sorted(SECTIONS)
    for name, lines in sections.items():
        (path / name).write_text("\n".join(lines) + "\n")
    return path


def stock_sections():
    return _read_bundle(Path(__file__).resolve().parent.parent / "open-msspe-design_amd" / "data" / "nn_params.bundle")


def _tokens(lines):
    return [t for line in lines for t in line.split()]


def _num(x: float) -> str:
    x = round(x, 6)
    return repr(int(x)) if x == int(x) else repr(x)


def _mapped(sections, edits):
    """edits: {section: f(flat index, value) -> new value or None (= 'inf')} over the finite entries; one token a line."""
    out = {name: list(lines) for name, lines in sections.items()}
    for name, f in edits.items():
        new = []
        for i, t in enumerate(_tokens(sections[name])):
            if t != "inf":
                v = f(i, float(t))
                t = "inf" if v is None else _num(v)
            new.append(t)
        out[name] = new
    return out


def wc_missing(s):
    """The AA/TT and TT/AA stacks do not exist: a Watson-Crick neighbour without a stack term.  thal.c never extends a
    helix over it; only the dense kernel restates that rule, so every other route stands down (csrc/nn_params.cpp
    fill_compact_planes)."""
    gone = lambda i, v: None if i in (15, 240) else v
    return _mapped(s, {"stack.ds": gone, "stack.dh": gone})


def dangle_holes(s):
    """Every third finite dangle is missing, so some closing pairs have only a 3' or only a 5' dangle."""
    finite = [i for i, t in enumerate(_tokens(s["dangle.ds"])) if t != "inf"]
    holes = set(finite[2::3])
    gone = lambda i, v: None if i in holes else v
    return _mapped(s, {"dangle.ds": gone, "dangle.dh": gone})


def loops_only(s):
    """Other interior, bulge and hairpin loop terms, still on the 0.01 cal/K and 10 cal grids (row k, column c of
    1 .. 3; token 4 k of the section is the loop size)."""
    ds = lambda i, v: v if i % 4 == 0 else v + 0.01 * ((i // 4 + i % 4) % 5 - 2)
    dh = lambda i, v: v if i % 4 == 0 else v + 10 * (((i // 4) * (i % 4)) % 7 - 3)
    return _mapped(s, {"loops.ds": ds, "loops.dh": dh})


_BONUS_STEP = {"triloop.ds": -0.37, "triloop.dh": 130.0, "tetraloop.ds": 0.11, "tetraloop.dh": -70.0}
_BONUS_ADDED = {"triloop.ds": ("ACGTT",), "triloop.dh": ("ACGTT", "CAAAG"), "tetraloop.ds": ("GACGTC",),
                "tetraloop.dh": ("GACGTC",)}
_BONUS_ADDED_VALUE = {"triloop.ds": -1.23, "triloop.dh": -2100.0, "tetraloop.ds": 2.4, "tetraloop.dh": -1800.0}


def _bonus_pairs(lines):
    t = _tokens(lines)
    return list(zip(t[0::2], t[1::2]))


def loops_and_bonuses(s):
    """loops_only, and the tri- and tetraloop bonuses: every fifth key dropped, the others shifted (triloop entropies
    leave zero), keys added out of order, one of them to the enthalpy file alone."""
    out = loops_only(s)
    for name in BONUS_SECTIONS:
        new = []
        for p, (key, val) in enumerate(_bonus_pairs(s[name])):
            if p % 5 == 4:
                continue
            new.append(f"{key}\t{_num(float(val) + _BONUS_STEP[name] * (p % 4 + 1))}")
        new += [f"{key}\t{_num(_BONUS_ADDED_VALUE[name])}" for key in _BONUS_ADDED[name]]
        out[name] = new
    return out


def _cap_keys():
    """Keys that fill the bonus tables to the caps of the device tables (32 and 128): T.A-closed loops that start with
    T, which sort behind every shipped key but TTTTGA and TTTTTA, so they sit in the slots the shipped tables leave
    empty."""
    s = stock_sections()
    tri = ["TT" + x + y + "A" for x in "ACGT" for y in "ACGT"]
    have = {k for k, _ in _bonus_pairs(s["tetraloop.dh"])}
    tet = [k for k in ("TT" + x + y + z + "A" for x in "ACGT" for y in "ACGT" for z in "ACGT") if k not in have][:51]
    return tri, tet


def bonus_caps(s):
    """loops_only with the bonus tables filled to their caps: the 16 and 77 shipped keys and 16 and 51 new ones, each
    with an entropy and an enthalpy of its own that favour the closure, written in front of the shipped keys."""
    out = loops_only(s)
    tri, tet = _cap_keys()
    out["triloop.ds"] = [f"{k}\t{_num(-0.5 - 0.07 * q)}" for q, k in enumerate(tri)] + out["triloop.ds"]
    out["triloop.dh"] = [f"{k}\t{_num(-1500 - 40 * q)}" for q, k in enumerate(tri)] + out["triloop.dh"]
    out["tetraloop.ds"] = [f"{k}\t{_num(-0.3 - 0.03 * q)}" for q, k in enumerate(tet)] + out["tetraloop.ds"]
    out["tetraloop.dh"] = [f"{k}\t{_num(-1700 - 20 * q)}" for q, k in enumerate(tet)] + out["tetraloop.dh"]
    assert len(_bonus_pairs(out["triloop.dh"])) == 32 and len(_bonus_pairs(out["tetraloop.dh"])) == 128
    return out


def caps_oligos(k):
    """GCGC + K + GCGC for the keys bonus_caps adds (k = 13: triloops, 14: tetraloops)."""
    return ["GCGC" + key + "GCGC" for key in _cap_keys()[k - 13]]


def _scaled_stack(factor):
    mul = lambda i, v: v * factor
    return lambda s: _mapped(s, {"stack.ds": mul, "stack.dh": mul})


def h_mod10(s):
    """Two stack enthalpies that are integers but no multiples of 10: only the dense kernel computes with them."""
    return _mapped(s, {"stack.dh": lambda i, v: v + 5 if i in (15, 240) else v})


def h_frac(s):
    """A stack enthalpy that is no integer: the engine refuses every dimer call."""
    return _mapped(s, {"stack.dh": lambda i, v: -10600.5 if i == 105 else v})


VARIANTS = {
    "stock": lambda s: {name: list(lines) for name, lines in s.items()},
    "wc_missing": wc_missing,
    "dangle_holes": dangle_holes,
    "loops_only": loops_only,
    "loops_and_bonuses": loops_and_bonuses,
    "bonus_caps": bonus_caps,
    "stack_x1.5": _scaled_stack(1.5),
    "stack_x3": _scaled_stack(3.0),
    "h_mod10": h_mod10,
    "h_frac": h_frac,
}

# pair tables ok, fast_ok, int_ok, row_ok, split_max_k, wave_max_k
EXPECTED_ROUTES = {
    "stock": (1, 1, 1, 1, 32, 32),
    "wc_missing": (1, 0, 0, 0, 0, 0),
    "dangle_holes": (1, 1, 1, 1, 32, 32),
    "loops_only": (1, 1, 1, 1, 32, 32),
    "loops_and_bonuses": (1, 1, 1, 1, 32, 32),
    "bonus_caps": (1, 1, 1, 1, 32, 32),
    "stack_x1.5": (1, 0, 0, 0, 21, 32),
    "stack_x3": (1, 0, 0, 0, 10, 28),
    "h_mod10": (1, 0, 0, 0, 0, 0),
    "h_frac": (0, 0, 0, 0, 0, 0),
}


# Rectangles and flanked site passes (tests/test_gpu_param_variants.py g to i, the stack_x3 cases of the reach tests):
# a row oligo against a column oligo or template of another length goes by the longer of the two, kmax.
COMPUTED = ("wc_missing", "dangle_holes", "loops_and_bonuses", "stack_x1.5", "stack_x3", "h_mod10")
RECT_ANY_ALWAYS = ((13, 20), (20, 13), (2, 17))
RECT_ANY_EXTRA = {
    "stack_x1.5": ((16, 21), (16, 22)),                                   # split_max_k and one above
    "stack_x3": ((8, 10), (8, 11), (20, 28), (20, 29), (29, 13)),         # either bound and one above; long rows
    "wc_missing": ((8, 32),),                                             # dense only, the widest table
    "h_mod10": ((8, 32),),
}
# where the longer oligo of an extra shape must sit: (bound, bases above it)
RECT_ANY_ON_BOUND = {
    ("stack_x1.5", 16, 21): ("split_max_k", 0), ("stack_x1.5", 16, 22): ("split_max_k", 1),
    ("stack_x3", 8, 10): ("split_max_k", 0), ("stack_x3", 8, 11): ("split_max_k", 1),
    ("stack_x3", 20, 28): ("wave_max_k", 0), ("stack_x3", 20, 29): ("wave_max_k", 1), ("stack_x3", 29, 13): ("wave_max_k", 1),
}
RECT_ANY_CASES = [(v, a, b) for v in COMPUTED for a, b in RECT_ANY_ALWAYS + RECT_ANY_EXTRA.get(v, ())]
RECT_END_SHAPES = ((13, 20), (20, 13), (20, 28), (20, 29))
FLANK_VARIANTS = ("wc_missing", "dangle_holes", "stack_x1.5", "stack_x3", "h_mod10")
FLANK_GRID = ((13, 2), (17, 1), (24, 4))                                  # (k, flank): templates of k .. k + 2 flank bases


def rect_stage(routes: dict, kmax: int, end: bool = False) -> str:
    """The first stage a rectangle takes at the default options (csrc/capi.cpp: cross_dimer_impl, and with end
    cross_dimer_end_impl and score_site_pairs, which have no split-table kernel): "split" up to split_max_k, else
    "wave" (one wave per pair) up to wave_max_k, else "dense"."""
    if not end and kmax <= routes["split_max_k"]:
        return "split"
    return "wave" if kmax <= routes["wave_max_k"] else "dense"


# {variant: ({kmax: stage} of the ANY rectangles, the same without the split kernel: END rectangles and templates)}
EXPECTED_RECT_STAGE = {
    "wc_missing": ({17: "dense", 20: "dense", 32: "dense"}, {20: "dense", 28: "dense", 29: "dense"}),
    "dangle_holes": ({17: "split", 20: "split"}, {20: "wave", 28: "wave", 29: "wave"}),
    "loops_and_bonuses": ({17: "split", 20: "split"}, {20: "wave", 28: "wave", 29: "wave"}),
    "stack_x1.5": ({17: "split", 20: "split", 21: "split", 22: "wave"}, {20: "wave", 28: "wave", 29: "wave"}),
    "stack_x3": ({10: "split", 11: "wave", 17: "wave", 20: "wave", 28: "wave", 29: "dense"},
                 {20: "wave", 28: "wave", 29: "dense"}),
    "h_mod10": ({17: "dense", 20: "dense", 32: "dense"}, {20: "dense", 28: "dense", 29: "dense"}),
}


def variant_sections(name):
    return VARIANTS[name](stock_sections())


def routes_tuple(routes: dict) -> tuple:
    return tuple(routes[k] for k in ("pair_tables", "fast_ok", "int_ok", "row_ok", "split_max_k", "wave_max_k"))


def bonus_pool():
    """GCGC + K + GCGC for every tri- and tetraloop key K that loops_and_bonuses keeps, drops or adds (K's first and
    last base close the loop): {"kept" | "dropped" | "added": {13: [...], 14: [...]}}."""
    s = stock_sections()
    pool = {c: {13: [], 14: []} for c in ("kept", "dropped", "added")}
    for name, k in (("triloop.dh", 13), ("tetraloop.dh", 14)):
        for p, (key, _) in enumerate(_bonus_pairs(s[name])):
            pool["dropped" if p % 5 == 4 else "kept"][k].append("GCGC" + key + "GCGC")
        pool["added"][k] += ["GCGC" + key + "GCGC" for key in _BONUS_ADDED[name]]
    return pool


def bonus_oligos(k):
    p = bonus_pool()
    return p["kept"][k] + p["dropped"][k] + p["added"][k]
