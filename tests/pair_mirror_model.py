"""A parameter bundle that is not strand-symmetric (test infrastructure, no GPU): what the mirrored bound first stage
(option pair_mirror) must refuse."""
import param_variants as pv


def broken_sections():
    """The stock bundle with the enthalpy of the stacked pair AC/TG raised by 100 cal/mol; its strand-swapped partner
    GT/CA keeps its value.  (stack.dh index ((a * 4 + b) * 4 + c) * 4 + d for the stack a b / c d.)"""
    a, b = 0, 1                                     # A, C on one strand, T, G opposite
    idx = ((a * 4 + b) * 4 + (3 - a)) * 4 + (3 - b)
    partner = (((3 - b) * 4 + (3 - a)) * 4 + b) * 4 + a
    assert idx != partner
    s = pv.stock_sections()
    toks = pv._tokens(s["stack.dh"])
    assert toks[idx] != "inf" and toks[idx] == toks[partner]
    return pv._mapped(s, {"stack.dh": lambda i, v: v + 100 if i == idx else v})
