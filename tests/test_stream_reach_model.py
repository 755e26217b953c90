"""The reach model (tests/stream_reach_model.py) against hand-worked cases: one site on each strand with D = k, D past
the record end, two sites D and D + 1 apart, a palindromic site, the tie rule, empty records, several primers at one
position, and the rendered block and CSV."""
import numpy as np

import background_model as bm
import stream_reach_model as srm

K = 5
U = "AACCG"                 # plus site where the stream reads AACCG, minus site where it reads CGGTT
RU = bm.revcomp(U)
PAL = "ACGT" + "ACGT"       # its own reverse complement (k = 8)


def fields(rec):
    return {f: int(rec[f]) for f in srm.FIELDS}


def one(records, primers, D, M=0, E=0):
    counts, stable, recs = srm.reach(None, records, primers, M, E, "any", 0.0, D)
    np.testing.assert_array_equal(counts, stable)
    return counts, recs


def test_one_site_each_strand_with_reach_k():
    #          0         1         2
    #          0123456789012345678901234
    record = "TTTTT" + U + "TTTTT" + RU + "TTTTT"
    assert RU == "CGGTT" and len(record) == 25
    counts, recs = one([record], [U], K)
    assert counts.tolist() == [[1, 1]]
    assert fields(recs[0]) == dict(sites_plus=1, sites_minus=1, reached_plus=5, reached_minus=5, reached_either=10,
                                   reached_both=0, gap_plus_len=15, gap_plus_pos=10, gap_minus_len=15, gap_minus_pos=0,
                                   gap_either_len=5, gap_either_pos=0)      # three runs of 5: the lowest wins
    # D = k + 2: the plus site reaches [5, 11], the minus site [13, 19]
    _c, recs = one([record], [U], K + 2)
    assert fields(recs[0]) == dict(sites_plus=1, sites_minus=1, reached_plus=7, reached_minus=7, reached_either=14,
                                   reached_both=0, gap_plus_len=13, gap_plus_pos=12, gap_minus_len=13, gap_minus_pos=0,
                                   gap_either_len=5, gap_either_pos=0)


def test_reach_past_the_record_end_stays_in_the_record():
    records = ["GGG" + U + "GG", "G" + RU + "GGGG", "GGGGGGGGGG"]
    starts = bm.record_starts(records)[0].tolist()
    assert starts == [0, 11, 22]
    _c, recs = one(records, [U], 1000)
    # record 0: a plus site at offset 3 reaches to the record's end, never into record 1
    assert fields(recs[0]) == dict(sites_plus=1, sites_minus=0, reached_plus=7, reached_minus=0, reached_either=7,
                                   reached_both=0, gap_plus_len=3, gap_plus_pos=0, gap_minus_len=10, gap_minus_pos=0,
                                   gap_either_len=3, gap_either_pos=0)
    # record 1: a minus site at offset 1 reaches from its last column (offset 5) down to the record's start
    assert fields(recs[1]) == dict(sites_plus=0, sites_minus=1, reached_plus=0, reached_minus=6, reached_either=6,
                                   reached_both=0, gap_plus_len=10, gap_plus_pos=11, gap_minus_len=4, gap_minus_pos=17,
                                   gap_either_len=4, gap_either_pos=17)
    # record 2: no site, every gap is the whole record
    assert fields(recs[2]) == dict(sites_plus=0, sites_minus=0, reached_plus=0, reached_minus=0, reached_either=0,
                                   reached_both=0, gap_plus_len=10, gap_plus_pos=22, gap_minus_len=10, gap_minus_pos=22,
                                   gap_either_len=10, gap_either_pos=22)


def test_two_sites_d_apart_leave_no_gap_and_d_plus_one_a_gap_of_one():
    D = 9
    for apart, gap in ((D, 0), (D + 1, 1)):
        record = U + "T" * (apart - K) + U + "T" * (D - K)      # the second site's reach ends with the record
        _c, recs = one([record], [U], D)
        f = fields(recs[0])
        assert f["sites_plus"] == 2 and f["reached_plus"] == len(record) - gap
        assert (f["gap_plus_len"], f["gap_plus_pos"]) == ((1, D) if gap else (0, 0))
        assert (f["gap_either_len"], f["gap_either_pos"]) == ((1, D) if gap else (0, 0))
        assert (f["gap_minus_len"], f["gap_minus_pos"]) == (len(record), 0)
    # the minus strand likewise: ends D apart
    for apart, gap in ((D, 0), (D + 1, 1)):
        record = "T" * (D - K) + RU + "T" * (apart - K) + RU
        _c, recs = one([record], [U], D)
        f = fields(recs[0])
        assert f["sites_minus"] == 2 and f["reached_minus"] == len(record) - gap
        assert (f["gap_minus_len"], f["gap_minus_pos"]) == ((1, D) if gap else (0, 0))


def test_a_palindromic_site_reaches_both_ways():
    record = "CCCCCC" + PAL + "CCCCCC"        # a site on both strands at offset 6
    counts, recs = one([record], [PAL], 10)
    assert counts.tolist() == [[1, 1]]
    # plus [6, 15], minus [4, 13]
    assert fields(recs[0]) == dict(sites_plus=1, sites_minus=1, reached_plus=10, reached_minus=10, reached_either=12,
                                   reached_both=8, gap_plus_len=6, gap_plus_pos=0, gap_minus_len=6, gap_minus_pos=14,
                                   gap_either_len=4, gap_either_pos=0)        # [0, 3] and [16, 19] tie: the lowest


def test_ties_go_to_the_lowest_position():
    record = "TTT" + U + "TTT" + U + "TTT"
    _c, recs = one([record], [U], K)
    f = fields(recs[0])
    assert (f["gap_plus_len"], f["gap_plus_pos"]) == (3, 0) and (f["gap_either_len"], f["gap_either_pos"]) == (3, 0)
    records = ["GG", record]
    _c, recs = one(records, [U], K)
    assert (int(recs[1]["gap_plus_len"]), int(recs[1]["gap_plus_pos"])) == (3, 3)


def test_empty_records_are_zero_at_their_start():
    records = ["", U, "", "", "TT", ""]
    starts = bm.record_starts(records)[0].tolist()
    assert starts == [0, 1, 7, 8, 9, 12]
    _c, recs = one(records, [U], K)
    for r in (0, 2, 3, 5):
        f = fields(recs[r])
        assert all(f[name] == (starts[r] if name.endswith("_pos") else 0) for name in srm.FIELDS)
    assert fields(recs[1])["reached_plus"] == 5 and fields(recs[1])["gap_plus_pos"] == 1      # len 0: pos = s_r
    assert fields(recs[4]) == dict(sites_plus=0, sites_minus=0, reached_plus=0, reached_minus=0, reached_either=0,
                                   reached_both=0, gap_plus_len=2, gap_plus_pos=9, gap_minus_len=2, gap_minus_pos=9,
                                   gap_either_len=2, gap_either_pos=9)


def test_several_primers_at_one_position_count_once_and_invalid_columns_are_columns():
    record = "NNN" + U + "NRN" + "TT"
    near = "TACCG"                                   # one mismatch from U at its first base
    counts, recs = one([record], [U, U, near], 8, M=1, E=0)
    assert counts[:, 0].tolist() == [1, 1, 1]
    f = fields(recs[0])
    assert f["sites_plus"] == 1 and f["reached_plus"] == 8 and (f["gap_plus_len"], f["gap_plus_pos"]) == (3, 0)
    assert f["reached_either"] == 8 and (f["gap_either_len"], f["gap_either_pos"]) == (3, 0)


def test_longest_false_run():
    t, f = True, False
    assert srm.longest_false_run(np.array([], dtype=bool)) == (0, 0)
    assert srm.longest_false_run(np.array([t, t])) == (0, 0)
    assert srm.longest_false_run(np.array([f, t, f, f, t, f, f])) == (2, 2)
    assert srm.longest_false_run(np.array([f, f, f])) == (3, 0)


def test_render_block_and_csv():
    records = ["TTTTT" + U + "TTTTT" + RU + "TTTTT", "", "GGGGGGGGGGGG"]
    _c, recs = one(records, [U], K)
    text = srm.render(["a", "b", "c"], records, recs, K, 0, 0)
    assert text == ("\nTarget reach (extension 5 bases; sites: up to 0 mismatches, last 0 bases exact):\n"
                    "  Total: 3 genomes, 37 columns, reached plus 5, minus 5, either 10, both 0\n"
                    "  Genomes with a gap above 5: 1\n"
                    "  Longest gaps, 3 genomes (name: offset, length):\n"
                    "    c: 0, 12\n    a: 0, 5\n    b: 0, 0\n")
    assert "stable: thal END1 t >= 30.00 C" in srm.render(["a", "b", "c"], records, recs, K, 0, 0, "end1", 30.0)
    csv = srm.render_csv(["a", "b", "c"], records, recs).splitlines()
    assert csv[0] == "name,columns," + ",".join(srm.FIELDS)
    assert csv[1] == "a,25,1,1,5,5,10,0,15,10,15,0,5,0"
    assert csv[2] == "b,0,0,0,0,0,0,0,0,0,0,0,0,0"
    assert csv[3] == "c,12,0,0,0,0,0,0,12,0,12,0,12,0"
