"""The amplicon model (tests/background_amplicon_model.py) against hand-built cases: stable records constructed
directly -- no thal, no site search -- and the answers worked out by hand from the rule in include/msspe_hip.h."""
import numpy as np

import background_amplicon_model as bam
import background_model as bm

K = 13


def sites(*rows):
    """rows of (primer, pos, strand)."""
    out = np.zeros(len(rows), dtype=bm.SITE_DTYPE)
    for i, (primer, pos, strand) in enumerate(rows):
        out[i] = (primer, pos, 0, strand)
    return out


def amps(*rows):
    return np.array(list(rows), dtype=bam.AMPLICON_DTYPE) if rows else np.zeros(0, dtype=bam.AMPLICON_DTYPE)


def check(n, recs, records, min_len, max_len, want_list, k=K):
    counts, total, lst = bam.pair_sites(n, k, recs, records, min_len, max_len)
    np.testing.assert_array_equal(lst, want_list)
    assert total == len(want_list)
    want = np.zeros((n, 2), dtype=np.uint64)
    for f, r, _p, _l in want_list.tolist():
        want[f, 0] += 1
        want[r, 1] += 1
    np.testing.assert_array_equal(counts, want)
    assert counts[:, 0].sum() == counts[:, 1].sum() == total
    return counts


ONE = ["A" * 1000]


def test_exactly_min_and_exactly_max():
    # plus at 100; minus at 100 + 50 - 13 (len 50 = min_len) and at 100 + 200 - 13 (len 200 = max_len)
    recs = sites((0, 100, 0), (1, 137, 1), (2, 287, 1))
    check(3, recs, ONE, 50, 200, amps((0, 1, 100, 50), (0, 2, 100, 200)))


def test_one_base_outside_each_bound():
    recs = sites((0, 100, 0), (1, 136, 1), (2, 288, 1))      # len 49 and len 201
    check(3, recs, ONE, 50, 200, amps())
    check(3, recs, ONE, 49, 201, amps((0, 1, 100, 49), (0, 2, 100, 201)))


def test_same_position_is_an_amplicon_of_length_k():
    recs = sites((0, 500, 0), (0, 500, 1))
    check(1, recs, ONE, K, 100, amps((0, 0, 500, K)))
    check(1, recs, ONE, K + 1, 100, amps())


def test_minus_site_before_the_plus_site_is_none():
    recs = sites((0, 500, 0), (1, 499, 1), (1, 400, 1))        # the primers point away from each other
    check(2, recs, ONE, K, 1000, amps())


def test_pair_across_a_record_separator():
    records = ["A" * 100, "C" * 100]                           # record 1 starts at 101
    recs = sites((0, 80, 0), (1, 101, 1), (1, 87, 1), (0, 102, 0), (1, 150, 1))
    # 80 -> 101 straddles the separator; 80 -> 87 ends flush with record 0 (87 + 13 = 100); 102 -> 150 lies in record 1
    check(2, recs, records, K, 500, amps((0, 1, 80, 20), (0, 1, 102, 61)))
    # one base further the minus window would hold the separator: never a site, and the model refuses it as well
    recs = sites((0, 80, 0), (1, 88, 1))
    check(2, recs, records, K, 500, amps())


def test_invalid_columns_inside_a_record_do_not_break_an_amplicon():
    records = ["A" * 100 + "N" * 7 + "R" + "A" * 100]
    recs = sites((0, 50, 0), (1, 150, 1))
    check(2, recs, records, K, 500, amps((0, 1, 50, 113)))


def test_one_primer_on_both_ends():
    recs = sites((0, 10, 0), (0, 200, 1))
    counts = check(1, recs, ONE, K, 300, amps((0, 0, 10, 203)))
    assert counts.tolist() == [[1, 1]]


def test_duplicate_primers_count_independently():
    # primers 0 and 1 are the same word: the same sites under both indices, and every combination is an amplicon
    recs = sites((0, 10, 0), (1, 10, 0), (0, 100, 1), (1, 100, 1))
    counts = check(2, recs, ONE, K, 300, amps((0, 0, 10, 103), (0, 1, 10, 103), (1, 0, 10, 103), (1, 1, 10, 103)))
    assert counts.tolist() == [[2, 2], [2, 2]]


def test_every_pair_of_several_sites_and_the_order_of_the_list():
    recs = sites((1, 30, 0), (0, 10, 0), (2, 60, 1), (0, 60, 1), (1, 40, 1))
    check(3, recs, ONE, K, 300, amps((0, 1, 10, 43), (0, 0, 10, 63), (0, 2, 10, 63), (1, 1, 30, 23), (1, 0, 30, 43),
                                     (1, 2, 30, 43)))


def test_empty_records():
    records = ["", "A" * 100, "", "", "C" * 100, ""]
    starts, total = bm.record_starts(records)
    assert starts.tolist() == [0, 1, 102, 103, 104, 205] and total == 205
    recs = sites((0, 1, 0), (1, 88, 1), (0, 80, 0), (1, 104, 1), (0, 105, 0), (1, 191, 1))
    # 1 -> 88 spans record 1 from its first to its last window, 80 -> 88 lies inside it; 1 -> 104 and 80 -> 104 cross
    # two empty records; 105 -> 191 ends flush with record 4 (191 + 13 = 204)
    check(2, recs, records, K, 500, amps((0, 1, 1, 100), (0, 1, 80, 21), (0, 1, 105, 99)))


def test_no_stable_sites_and_no_records():
    check(3, sites(), ONE, K, 500, amps())
    check(3, sites((0, 5, 0), (1, 7, 0)), ONE, K, 500, amps())     # plus sites only
    check(0, sites(), [], K, 500, amps())


def test_only_stable_records_are_paired():
    import background_thal_model as btm
    recs = np.zeros(3, dtype=btm.SCORED_SITE_DTYPE)
    recs["primer"], recs["pos"], recs["strand"], recs["stable"] = [0, 1, 1], [10, 100, 120], [0, 1, 1], [1, 0, 1]
    counts, total, lst = bam.amplicons_of(2, K, recs, ONE, K, 300)
    np.testing.assert_array_equal(lst, amps((0, 1, 10, 123)))
    assert total == 1 and counts.tolist() == [[1, 0], [0, 1]]


def test_render():
    records = ["A" * 100, "C" * 100]
    recs = sites((0, 10, 0), (1, 50, 1), (1, 120, 0), (0, 150, 1))
    counts, _total, lst = bam.pair_sites(2, K, recs, records, K, 300)
    text = bam.render(["Primer_0_F", "Primer_0_R"], ["b0", "b1"], records, counts, lst, K, 300)
    assert text == ("\nBackground amplicons (stable sites facing each other, 13 to 300 bases):\n"
                    "  Primer_0_F: as forward 1, as reverse 1\n"
                    "  Primer_0_R: as forward 1, as reverse 1\n"
                    "  Total: 2 primers, 2 amplicons\n"
                    "  First 2 (record:offset, length, forward, reverse):\n"
                    "    b0:10, 53, Primer_0_F, Primer_0_R\n"
                    "    b1:19, 43, Primer_0_R, Primer_0_F\n")
