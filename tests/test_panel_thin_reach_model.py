"""The reach-thinning model (tests/panel_thin_reach_model.py) against hand-worked cases: the tie rule, a union that is
not a sum, a clipped plus interval with a minus interval nested inside it, a word listed twice, a forced primer that
covers another's set, min_gain ending the loop early, a primer without a site, empty records, and the rendered block."""
import numpy as np

import background_model as bm
import panel_thin_reach_model as trm
import stream_reach_model as srm

K = 5
U = "AACCG"                 # plus site where the stream reads AACCG, minus site where it reads CGGTT
RU = bm.revcomp(U)
V = "GATTC"                 # minus site where the stream reads GAATC
W = "ACCGA"                 # overlaps U by four bases in AACCGA


def one(records, primers, D, min_gain=1, forced=None, M=0, E=0):
    return trm.thin(None, records, primers, M, E, "any", 0.0, D, min_gain, forced)


def test_equal_reach_goes_to_the_lower_index():
    record = U + "TTTTT" + V + "TTTTT"
    for primers in ([U, V], [V, U]):
        r = one([record], primers, K)
        assert r["primer_reach"].tolist() == [5, 5]
        assert r["order"].tolist() == [0, 1] and r["gains"].tolist() == [5, 5] and r["keep"].tolist() == [1, 1]
        assert r["reached_all"] == r["reached_kept"] == 10


def test_sites_closer_than_the_reach_count_their_union():
    #         0123456789
    record = U + "T" + U + "T" * 10          # sites at 0 and 6, D = 8: [0, 7] and [6, 13]
    r = one([record], [U], 8)
    assert r["counts"].tolist() == [[2, 0]]
    assert r["primer_reach"].tolist() == [14] and r["gains"].tolist() == [14] and r["reached_all"] == 14
    assert int(r["records"][0]["reached_plus"]) == 14


def test_a_clipped_plus_interval_holds_a_minus_interval():
    record = U + "T" + RU + "TT"            # 13 columns; plus site at 0, minus site at 6
    r = one([record], [U], 100)             # plus [0, 12] cut at the record's end, minus [0, 10] cut at its start
    assert r["counts"].tolist() == [[1, 1]]
    assert r["primer_reach"].tolist() == [13] and r["gains"].tolist() == [13]
    rec = r["records"][0]
    assert (int(rec["reached_plus"]), int(rec["reached_minus"]), int(rec["reached_both"])) == (13, 11, 11)
    # in a second record the same primer reaches on: its sets never leave their records
    r = one([record, "TT" + U], [U], 100)
    assert r["primer_reach"].tolist() == [13 + 5] and r["reached_all"] == 18


def test_a_word_listed_twice_is_picked_once():
    record = U + "TTTTT" + V + "TTTTT"
    r = one([record], [U, V, U], 7)
    assert r["primer_reach"].tolist() == [7, 7, 7]
    assert r["order"].tolist() == [0, 1] and r["gains"].tolist() == [7, 7] and r["keep"].tolist() == [1, 1, 0]
    assert r["reached_all"] == r["reached_kept"] == 14
    np.testing.assert_array_equal(r["records"], one([record], [U, V], 7)["records"])


def test_a_forced_primer_that_covers_another():
    record = U + "TT" + "GAATC"              # V's minus site ends the record: it reaches [12 - D, 11]
    r = one([record], [U, V], 12, forced=[1, 0])      # U reaches [0, 11], the whole record
    assert r["primer_reach"].tolist() == [12, 12]     # V's [0, 11] is cut at the record's start
    assert r["order"].tolist() == [] and r["keep"].tolist() == [1, 0]
    assert r["reached_all"] == r["reached_kept"] == 12
    r = one([record], [U, V], 6, forced=[1, 0])       # U [0, 5], V [6, 11]: now V adds six columns
    assert r["order"].tolist() == [1] and r["gains"].tolist() == [6] and r["keep"].tolist() == [1, 1]
    r = one([record], [U, V], 6, forced=[0, 1])       # a forced primer is never in the order
    assert r["order"].tolist() == [0] and r["keep"].tolist() == [1, 1]
    r = one([record], [U, V], 6, forced=[1, 1])
    assert r["order"].tolist() == [] and r["reached_kept"] == 12


def test_min_gain_two_ends_the_loop_early():
    record = "AACCGA" + "TTTT"               # U at 0 reaches [0, 4], W at 1 reaches [1, 5]: W adds one column
    r = one([record], [U, W], K, min_gain=1)
    assert r["order"].tolist() == [0, 1] and r["gains"].tolist() == [5, 1] and r["reached_kept"] == 6
    r = one([record], [U, W], K, min_gain=2)
    assert r["order"].tolist() == [0] and r["gains"].tolist() == [5] and r["keep"].tolist() == [1, 0]
    assert (r["reached_all"], r["reached_kept"]) == (6, 5)
    assert int(r["records"][0]["reached_either"]) == 5 and int(r["records"][0]["sites_plus"]) == 1
    r = one([record], [U, W], K, min_gain=6)
    assert r["order"].tolist() == [] and r["keep"].tolist() == [0, 0] and r["reached_kept"] == 0
    assert int(r["records"][0]["gap_either_len"]) == 10


def test_a_primer_without_a_site_is_never_picked():
    record = U + "TTTTT"
    r = one([record], ["GGGGG", U], K)
    assert r["counts"].tolist() == [[0, 0], [1, 0]]
    assert r["primer_reach"].tolist() == [0, 5] and r["order"].tolist() == [1] and r["keep"].tolist() == [0, 1]
    r = one([record], ["GGGGG"], K)
    assert r["order"].tolist() == [] and r["reached_all"] == 0 and int(r["records"][0]["gap_either_len"]) == 10


def test_empty_records():
    records = ["", U + "TT", "", RU]
    starts = bm.record_starts(records)[0].tolist()
    assert starts == [0, 1, 9, 10]
    r = one(records, [U], 6)
    assert r["primer_reach"].tolist() == [6 + 5] and r["reached_all"] == 11      # [1, 6] and [10, 14], cut at its start
    for i in (0, 2):
        assert all(int(r["records"][i][f]) == (starts[i] if f.endswith("_pos") else 0) for f in srm.FIELDS)


def test_rendered_block():
    record = "AACCGA" + "TTTT"
    r = one([record], [U, W], K, min_gain=2)
    assert trm.render(r, K, 2, 0, 0) == ("\nReach thinning (extension 5 bases, min gain 2; sites: up to 0 mismatches, "
                                         "last 0 bases exact):\n"
                                         "  Kept 1 of 2 primers (0 forced)\n"
                                         "  Columns reached by all: 6, by kept: 5\n")
    text = trm.render(r, K, 2, 1, 2, "end1", 30.0, forced=[0, 1])
    assert "stable: thal END1 t >= 30.00 C" in text and "(1 forced)" in text
