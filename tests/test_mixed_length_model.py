"""Pools of different oligo lengths, without a GPU: the C ABI and Python surface of the A x B screen exist, and
the long-oligo integer recurrence of csrc/thal_pairs_split.hip restated for a RECTANGULAR table (row oligo of k1
bases, column oligo of k2) over the tables the kernel keeps in LDS (msspe_host_split_tables) reproduces the
oracle's fillMatrix planes.  This pins the exactness argument for k1 != k2 before the GPU runs it."""
import ctypes as C

import numpy as np
import pytest

import int_dp_model
import split_dp_model as model

NEW_SYMBOLS = ("msspe_cross_dimer_ab_dev", "msspe_cross_dimer_ab_edges_dev", "msspe_cross_dimer_ab",
               "msspe_cross_dimer_edges_mixed")


def test_symbols_and_methods_exist():
    import msspe_amd
    from msspe_amd import capi
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes, name   # resolved in the library, typed by the binding
    for meth in ("cross_dimer_ab", "cross_dimer_ab_edges", "cross_dimer_ab_dev", "cross_dimer_edges_mixed",
                 "cross_dimer_ab_edges_dev"):
        assert callable(getattr(msspe_amd.Engine, meth))


def test_ab_calls_check_arguments_before_any_device_work():
    """A null context is refused without touching a device."""
    from msspe_amd import capi
    lib = capi.load_library()
    chem = capi.Chem.ntthal()
    assert lib.msspe_cross_dimer_ab(None, b"ACGT", 1, 4, b"ACG", 1, 3, C.byref(chem), C.c_float(-9000.0),
                                    None, None, None, None) == 1
    assert lib.msspe_cross_dimer_edges_mixed(None, None, 0, C.byref(chem), C.c_float(-9000.0), None, 0,
                                             None) == 1


def cell_bases_rect(s1, s2, im1, jm1):
    """split_dp_model.cell_bases with the right-end neighbours bounded by each oligo's own length."""
    a = s1[im1]
    oaL = s1[im1 - 1] if im1 > 0 else 4
    oaR = s1[im1 + 1] if im1 < len(s1) - 1 else 4
    obL = s2[jm1 - 1] if jm1 > 0 else 4
    obR = s2[jm1 + 1] if jm1 < len(s2) - 1 else 4
    ci = (((3 - a) * 4 + (obL & 3)) * 4 + (oaL & 3)) & 63
    return dict(a=a, idxL=model.K_ENDL + a * 25 + oaL * 5 + obL, idxR=model.K_ENDR + a * 25 + oaR * 5 + obR,
                wc=model.K_WC + (oaL & 3) * 4 + a, po=a | ((oaR & 3) << 2) | ((obR & 3) << 4),
                yTS=model.K_TSC + ci, yMM=model.K_MMC + ci, bBase=model.K_BU + a * model.K_BUSTRIDE)


def run_pair_rect(tb, init_S, RC, a, b):
    """split_dp_model.run_pair for len(a) != len(b): cells over i < k1, j < k2 in row-major order."""
    s1 = [model.CODE[c] for c in a]
    s2 = [model.CODE[c] for c in reversed(b)]
    k1, k2 = len(a), len(b)
    cells, order, hard = {}, [], False
    for im1 in range(k1):
        for jm1 in range(k2):
            if s1[im1] + s2[jm1] != 3:
                continue
            cb = cell_bases_rect(s1, s2, im1, jm1)
            cgeo = (im1 - 1) * 32 + (jm1 - 1)
            jm1p = jm1 - 1
            yTS, yMM = int(tb.g[cb["yTS"]]), int(tb.g[cb["yMM"]])
            bestG, winners, stk = model.K_VALID, [], None
            for (pi, pj) in order:
                Gp, Hp, po = cells[(pi, pj)]
                d = cgeo - (pi * 32 + pj)
                if not (pj <= jm1p and d >= 0):
                    continue
                if d == 0:
                    stk = (Gp, Hp)
                l1z, l2z = d < 32, pj == jm1p
                pe = (po & 3) | (cb["a"] << 2)
                if l1z or l2z:
                    xi = (model.K_XB1 + d * 16 + pe) if l1z else (model.K_XB2 + (d >> 5) * 16 + pe)
                    y = 0
                elif d == 0x21:
                    xi, y = model.K_XMM + po, yMM
                else:
                    xi, y = model.K_XP + po, yTS
                cand = int(tb.L[d]) + int(tb.X[xi]) + y + Gp
                if cand < bestG:
                    bestG, winners = cand, [(pi, pj, po, Hp)]
                elif cand == bestG:
                    winners.append((pi, pj, po, Hp))
            H0, G0 = int(tb.H[cb["idxL"]]), int(tb.g[cb["idxL"]])
            if stk is not None:
                rS, rH = float(tb.S[cb["idxR"]]), int(tb.H[cb["idxR"]])
                H1, G1 = stk[1] + int(tb.H[cb["wc"]]), stk[0] + int(tb.g[cb["wc"]])
                A0, A1 = float(H0 + 200 + rH), float(H1 + 200 + rH)
                B0 = ((model.entropy_of(G0, H0) + init_S) + rS) + RC
                B1 = ((model.entropy_of(G1, H1) + init_S) + rS) + RC
                lhs, rhs = A1 * B0, A0 * B1
                if not (B0 < 0 and B1 < 0 and abs(lhs - rhs) > 1e-9 * (abs(lhs) + abs(rhs))):
                    hard = True
                if lhs > rhs:
                    H0, G0 = H1, G1

            def enthalpy(w):
                pi, pj, po, Hp = w
                l1, l2 = im1 - 1 - pi, jm1 - 1 - pj
                sz = l1 + l2
                if min(l1, l2) == 0:
                    lx, yidx = sz * 4 + (po & 3) + cb["bBase"], model.K_ZERO
                else:
                    lx = sz * 64 + po + (model.K_NB - 2 * 64)
                    yidx = cb["yMM"] if (l1, l2) == (1, 1) else cb["yTS"]
                return int(tb.H[lx]) + int(tb.H[yidx]) + Hp

            if bestG < G0:
                hs = {enthalpy(w) for w in winners}
                if len(winners) > 2 or len(hs) > 1:
                    hard = True
                Hw = enthalpy(winners[0])
                if Hw > 0 and 2000 * Hw - bestG > -1000:
                    hard = True
                H0, G0 = Hw, bestG
            elif bestG == G0 and enthalpy(winners[0]) != H0:
                hard = True
            cells[(im1, jm1)] = (G0, H0, cb["po"])
            order.append((im1, jm1))
    return cells, hard


@pytest.fixture(scope="module")
def tables():
    import msspe_amd
    return model.load_tables(msspe_amd)


@pytest.fixture(scope="module")
def consts():
    import msspe_amd
    tb = int_dp_model.load_tables(msspe_amd)
    return tb.init_S, tb.RC


def _random_oligo(rng, k):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, k))


def test_equal_lengths_restate_the_square_model(tables, consts):
    """k1 == k2: the rectangular restatement is the square one (tests/split_dp_model.py) cell for cell."""
    rng = np.random.default_rng(7)
    for k in (13, 20, 26):
        for _ in range(6):
            a, b = _random_oligo(rng, k), _random_oligo(rng, k)
            assert run_pair_rect(tables, consts[0], consts[1], a, b) == model.run_pair(tables, consts[0], consts[1], a, b)


def test_rectangular_recurrence_matches_oracle_planes(tables, consts, oracle, oracle_tables):
    """A few hundred random (k1, k2) shapes up to the tables' proven length, with constructed complementary pairs
    among them: every complementary cell's exact integer value equals the oracle's plane entry."""
    args = oracle.ntthal_args()
    rng = np.random.default_rng(2024)
    kmax = tables.max_k
    n_pairs, hard = 300, 0
    for t in range(n_pairs):
        k1, k2 = (int(x) for x in rng.integers(2, kmax + 1, 2))
        if k1 == k2:
            k2 = 2 + (k2 - 1) % (kmax - 1)
        a = _random_oligo(rng, k1)
        if t % 3 == 0 and k2 <= k1:
            # b holds the reverse complement of a substring of a: long helices, loops beside them
            at = int(rng.integers(0, k1 - k2 + 1))
            b = oracle.reverse_complement(a[at:at + k2])
        else:
            b = _random_oligo(rng, k2)
        cells, is_hard = run_pair_rect(tables, consts[0], consts[1], a, b)
        S, H = oracle.dimer_planes(oracle_tables, a, b, args)
        assert S.shape == (k1, k2)
        assert len(cells) == int(np.isfinite(H).sum()), (a, b)
        if is_hard:
            hard += 1       # the kernel hands such a pair to the f64 kernel
            continue
        for (i, j), (G, Hc, _po) in cells.items():
            assert Hc == H[i, j], (a, b, i, j)
            assert abs((2000.0 * H[i, j] - 620300.0 * S[i, j]) - G) < 0.5, (a, b, i, j)
    assert hard < 0.2 * n_pairs
