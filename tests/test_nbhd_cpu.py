"""Scylla's neighbourhoods on the CPU: the plain-Python statement (tests/nbhd_ref.py, transcribed from the C#) reproduces the assertions of
the reference's own tests as data (tests/golden/README_nbhd.md), and the host entry pisces_hip_nbhd_build equals the statement as whole
arrays on the fixtures, the named cases and 20 000 seeded rows.  tests/test_nbhd_gpu.py holds the device entry to both."""
import os

import numpy as np
import pytest

from pisces_amd import _abi, engine
from pisces_amd._native import PiscesHipError
from tests import nbhd_cases as N
from tests import nbhd_ref as ref

AT = lambda *positions: [(p, "A", "T") for p in positions]
# VcfNeighborhoodBuilderTests.GetNeighborhoods, every CreateNbhdBuilder call in order (phasingDistance 2, passingOnly true and
# minPassingVariantsInNbhd 0 unless given), and ForcedReport_alleles_are_not_included_in_neighborhood's:
# (fixture, criteria, rawNumNeighborhoods, the members CheckNeighborhoodVariants names, in the order of neighborhoods)
BUILDER_CONFIGURATIONS = [
    ("NbhdBuilderTest0", {}, 0, []),
    ("NbhdBuilderTest1", {}, 1, [AT(123, 124)]),
    ("NbhdBuilderTest2", {}, 1, [AT(123, 124, 125)]),
    ("NbhdBuilderTest3", {}, 2, [AT(123, 124, 125), AT(128, 129)]),
    ("NbhdBuilderTest4", {"distance": 5}, 1, [AT(123, 124, 128, 129)]),
    ("NbhdBuilderTest5", {}, 2, [AT(123, 124), AT(128, 129)]),
    ("NbhdBuilderTest5", {"distance": 5}, 1, [AT(123, 124, 128, 129)]),
    ("NbhdBuilderTest5", {"passing_only": False}, 2, [AT(123, 124, 125), AT(128, 129)]),
    ("NbhdBuilderTest5", {"distance": 5, "passing_only": False}, 1, [AT(123, 124, 125, 128, 129)]),
    ("NbhdBuilderTest5", {"passing_only": False, "min_passing": 1}, 2, [AT(123, 124, 125), AT(128, 129)]),
    ("NbhdBuilderTest5", {"passing_only": False, "min_passing": 2}, 2, [AT(123, 124, 125), AT(128, 129)]),
    ("NbhdBuilderTest5", {"passing_only": False, "min_passing": 3}, 2, [AT(128, 129)]),
    ("NbhdBuilderTest5", {"passing_only": False, "min_passing": 4}, 2, [AT(128, 129)]),
    ("NbhdBuilderForcedGT", {"distance": 10}, 1, [[(3751646, "C", "T"), (3751650, "AG", "A")]]),
]


def both(recs, pairs, kw, reference=None, batch_size=ref.UNBOUNDED):
    """(the statement's tables, the host entry's), compared as whole arrays"""
    statement_criteria, criteria = N.criteria_pair(**kw)
    want = N.statement(recs, pairs, statement_criteria, reference, batch_size)
    got = engine.nbhd_build(recs, pairs, criteria, reference)
    N.assert_same(got, want, "host entry")
    return want, got


@pytest.mark.parametrize("fixture,kw,raw,expected", BUILDER_CONFIGURATIONS, ids=[f"{i}-{c[0]}" for i, c in enumerate(BUILDER_CONFIGURATIONS)])
def test_get_neighborhoods(fixture, kw, raw, expected):
    rows = N.rows_of_vcf(fixture)
    want = N.statement(*N.make_rows(rows), N.criteria_pair(**{"distance": 2, **kw})[0])
    assert want["n_out"][4] == raw and want["n_out"][0] == len(expected)
    assert N.members(want) == expected
    in_order, descends_at = N.ascending(rows)
    if descends_at is not None:   # NbhdBuilderTest3's last line (125 behind 129): refused by name, the lines in front of it give the same neighbourhoods
        with pytest.raises(PiscesHipError) as e:
            engine.nbhd_build(*N.make_rows(rows), N.criteria_pair(**{"distance": 2, **kw})[1])
        assert e.value.n_out == (_abi.E_INVALID_ARG, 0, descends_at, 0, 0, 0)
    _, got = both(*N.make_rows(in_order), {"distance": 2, **kw})
    assert N.members(got) == expected and got["n_out"][4] == raw


def test_get_neighborhoods_from_messy_vcf():
    recs, pairs = N.make_rows(N.rows_of_vcf("VeryMutated"))
    want, _ = both(recs, pairs, {"distance": 2})
    assert want["n_out"][0] == 1 and want["n_out"][4] == 1 and want["n_out"][1] == 12


def test_forced_report_alleles_are_not_included():
    recs, pairs = N.make_rows(N.rows_of_vcf("NbhdBuilderForcedGT"))
    want, got = both(recs, pairs, {"distance": 10})
    assert [s[0] for s in N.members(want)[0]] == [3751646, 3751650] and N.members(want)[0][1][2] == "A"
    forced = [i for i, rec in enumerate(recs) if (int(rec["filter_bits"]) >> _abi.FILTER_FORCED_REPORT) & 1]
    assert len(forced) == 3 and all(got["row_class"][i] == _abi.NBHD_ROW_FORCED for i in forced)


def test_create_callable_nbhds_without_a_genome():
    """CreateCallableNbhdsTests, tests 1 and 2: new VcfNeighborhood(0, "chr1", new VariantSite(123), new VariantSite(125)) gives "RRR" """
    sites = []
    for p in (123, 125):
        s = ref.VariantSite()
        s.position, s.ref, s.alt, s.reference_name = p, "N", "N", "chr1"
        sites.append(s)
    c = ref.CallableNeighborhood(ref.VcfNeighborhood(0, "chr1", *sites))
    assert c.reference_substring == "RRR" and len(c.vcf.sites) == 2
    recs, pairs = N.make_rows([(123, "N", "N", N.HET, 0), (125, "N", "N", N.HET, 0)])
    _, got = both(recs, pairs, {})
    assert bytes(got["ref_bytes"]) == b"RRR" and N.members(got) == [[(123, "N", "N"), (125, "N", "N")]]


@pytest.mark.parametrize("fixture", N.FIXTURES)
def test_fixtures_at_every_batch_size(fixture):
    """_maxNumNbhdsInBatch and the hanging neighbourhood decide which call returns a neighbourhood, nothing else; the host entry equals
    the unbounded statement as whole arrays"""
    recs, pairs = N.make_rows(N.ascending(N.rows_of_vcf(fixture))[0])
    for kw in ({}, {"distance": 2}, {"distance": 5, "passing_only": False}, {"distance": 3, "passing_only": False, "min_passing": 3}):
        want, _ = both(recs, pairs, kw)
        for batch_size in (1, 2, 10):
            bounded = N.statement(recs, pairs, N.criteria_pair(**kw)[0], None, batch_size)
            assert N.members(bounded) == N.members(want) and bounded["n_out"] == want["n_out"]
            for k in ("sites", "alleles", "site_row", "site_original", "neighbourhoods", "ref_bytes", "row_class"):
                assert bounded[k].tobytes() == want[k].tobytes(), (batch_size, k)


def test_seeded_rows_at_every_batch_size():
    for seed in range(40):
        recs, pairs = N.make_rows(N.seeded_rows(seed, distance=10))
        kw = {**N.seeded_criteria(seed), "distance": 10}
        want = N.statement(recs, pairs, N.criteria_pair(**kw)[0])
        for batch_size in (1, 2, 10):
            bounded = N.statement(recs, pairs, N.criteria_pair(**kw)[0], None, batch_size)
            assert bounded["n_out"] == want["n_out"], (seed, batch_size)
            for k in ("sites", "alleles", "site_row", "site_original", "neighbourhoods", "ref_bytes", "row_class"):
                assert bounded[k].tobytes() == want[k].tobytes(), (seed, batch_size, k)


def test_chr21_is_one_neighbourhood_of_the_scylla_fixtures_49_sites():
    z = np.load(os.path.join(N.GOLDEN, "bam_scylla_chr21.npz"))
    rows = N.rows_of_vcf("chr21_11085587_S1")
    variants = [r for r in rows if r[2] != "."]
    assert len(variants) == 49 and all(r[3] == N.HET and r[4] == 0 for r in variants)          # all PASS and 0/1
    assert max(b[0] - a[0] for a, b in zip(variants, variants[1:])) == 11                       # the largest gap
    recs, pairs = N.make_rows(rows)
    want, got = both(recs, pairs, {})
    assert got["n_out"][:2] == (1, 49) and got["n_out"][4] == 1
    assert N.members(got)[0] == [(int(p), str(r), str(a)) for p, r, a in zip(z["vcf_position"], z["vcf_ref"], z["vcf_alt"])]
    assert list(got["site_row"]) == list(got["site_original"]) == [i for i, r in enumerate(rows) if r[2] != "."]   # stable order is file order here


def test_bounds_equal_the_read_passes():
    for name in ("mixed_group_of_five", "the_comments_insertion_before_snv", "a_far_eligible_row_breaks_the_chain"):
        recs, pairs, kw = N.named(name)
        _, got = both(recs, pairs, kw)
        assert len(got["info"]) > 0
        for (b, e), info, nb in zip(got["neighbourhoods"], got["info"], N.members(got)):
            assert engine.vead_neighborhood_info(nb) == (info["first"], info["last_with_look_ahead"], info["soft_clip_end_before"], info["soft_clip_pos_after"])
            assert info["last_in_vcf"] == nb[-1][0] and info["ref_len"] == info["last_with_look_ahead"] - info["first"]


def test_reference_substring():
    recs, pairs, kw = N.named("a_far_eligible_row_breaks_the_chain")   # neighbourhoods at 100, 130 and 200
    reference = ("ACGT" * 60)[:203]                                    # reaches the first two; the third's look-ahead 205 lies past its end
    want, got = both(recs, pairs, kw, reference.encode())
    text = bytes(got["ref_bytes"]).decode()
    assert [text[i["ref_offset"]:i["ref_offset"] + i["ref_len"]] for i in got["info"]] == [reference[99:104], reference[129:134], "RRRRR"]
    _, bare = both(recs, pairs, kw)
    assert bytes(bare["ref_bytes"]) == b"R" * 15


def test_the_comments_insertion_is_reordered_and_the_original_allele_is_not():
    recs, pairs, kw = N.named("the_comments_insertion_before_snv")
    _, got = both(recs, pairs, kw)
    assert N.members(got) == [[(140453137, "C", "T"), (140453137, "C", "CGTA"), (140453140, "G", "A")]]
    assert list(got["site_row"]) == [2, 1, 3] and list(got["site_original"]) == [1, 2, 3]
    assert [s != o for s, o in zip(got["site_row"], got["site_original"])] == [True, True, False]   # they differ exactly there
    assert list(got["sites"]["allele_offset"]) == [0, 2, 7] and bytes(got["alleles"]) == b"CTCCGTAGA"


def test_an_insertion_then_an_snv_one_base_on_keeps_its_place():
    recs, pairs, kw = N.named("an_insertion_then_an_snv_one_base_on")
    _, got = both(recs, pairs, kw)
    assert list(got["site_row"]) == list(got["site_original"]) == [0, 1]   # equal keys (101), input order


def test_mixed_group_of_five():
    recs, pairs, kw = N.named("mixed_group_of_five")
    _, got = both(recs, pairs, kw)
    assert list(got["site_row"]) == [1, 3, 4, 0, 2, 6, 5] and list(got["site_original"]) == [0, 1, 2, 3, 4, 5, 6]
    assert (got["info"]["n_passing"][0], got["info"]["n_non_passing"][0]) == (6, 1)


def test_ref_and_nocall_is_eligible():
    recs, pairs, kw = N.named("ref_and_nocall_is_eligible")
    _, got = both(recs, pairs, kw)
    assert list(got["row_class"]) == [_abi.NBHD_ROW_KEPT, _abi.NBHD_ROW_KEPT, _abi.NBHD_ROW_INELIGIBLE]


def test_phase_bits_do_not_fail_a_row():
    recs, pairs, kw = N.named("phase_bits_do_not_fail_a_row")
    _, got = both(recs, pairs, kw)
    assert got["n_out"][:2] == (1, 3) and (got["info"]["n_passing"][0], got["info"]["n_non_passing"][0]) == (3, 0)


def test_an_ineligible_row_between():
    recs, pairs, kw = N.named("an_ineligible_row_between")
    _, got = both(recs, pairs, kw)
    assert [[s[0] for s in nb] for nb in N.members(got)] == [[100, 108]]
    assert list(got["row_class"]) == [_abi.NBHD_ROW_KEPT, _abi.NBHD_ROW_INELIGIBLE, _abi.NBHD_ROW_KEPT, _abi.NBHD_ROW_LONE, _abi.NBHD_ROW_INELIGIBLE, _abi.NBHD_ROW_LONE]


def test_a_far_eligible_row_breaks_the_chain():
    recs, pairs, kw = N.named("a_far_eligible_row_breaks_the_chain")
    _, got = both(recs, pairs, kw)
    assert [[s[0] for s in nb] for nb in N.members(got)] == [[100, 104], [130, 134], [200, 204]]


def test_distance_exactly_the_phasing_distance_does_not_chain():
    recs, pairs, kw = N.named("distance_exactly_the_phasing_distance")
    _, got = both(recs, pairs, kw)
    assert [[s[0] for s in nb] for nb in N.members(got)] == [[110, 119]] and got["row_class"][0] == _abi.NBHD_ROW_LONE


def test_all_passing_below_the_minimum():
    """two passing rows under a minimum of three are kept, one passing and one failing are dropped; the dropped one keeps its number"""
    recs, pairs, kw = N.named("all_passing_below_the_minimum")
    _, got = both(recs, pairs, kw)
    assert [[s[0] for s in nb] for nb in N.members(got)] == [[100, 101], [300, 301]]
    assert list(got["info"]["raw_index"]) == [0, 2] and got["n_out"][4] == 3
    assert list(got["row_class"]) == [4, 4, 3, 3, 4, 4]


@pytest.mark.parametrize("name", ["distance_zero", "distance_negative"])
def test_no_distance_no_neighbourhood(name):
    recs, pairs, kw = N.named(name)
    _, got = both(recs, pairs, kw)
    assert got["n_out"] == (0, 0, 0, 0, 0, 3) and list(got["row_class"]) == [_abi.NBHD_ROW_LONE] * 3


@pytest.mark.parametrize("name", ["co_located_rows_chain", "het_only_drops_hom_alt", "a_forced_row_is_no_last_site", "an_unsupported_category"])
def test_further_named_cases(name):
    recs, pairs, kw = N.named(name)
    _, got = both(recs, pairs, kw)
    expected = {"co_located_rows_chain": [[100, 100]], "het_only_drops_hom_alt": [], "a_forced_row_is_no_last_site": [],
                "an_unsupported_category": [[100, 103]]}[name]
    assert [[s[0] for s in nb] for nb in N.members(got)] == expected


N_SEEDED_LISTS = 160
COUNTED = ["ineligible_reference", "ineligible_nocall", "ineligible_unsupported", "ineligible_hom_alt", "ineligible_filtered", "forced_skip", "chain_start", "append",
           "break_by_distance", "drop_by_minimum", "reorder", "nbhd_above_16", "nbhd_above_256"]


def test_seeded_rows_host_entry_equals_the_statement():
    """at least 20 000 rows in lists of 0 to 400, each criterion drawn both ways, every counted branch of the statement taken 20 times"""
    ref.COUNTS.clear()
    total, drawn = 0, {k: set() for k in ("distance", "passing_only", "het_only", "min_passing")}
    for seed in range(N_SEEDED_LISTS):
        kw = N.seeded_criteria(seed)
        recs, pairs = N.make_rows(N.seeded_rows(seed, distance=kw["distance"]))
        both(recs, pairs, kw)
        total += len(recs)
        for k in drawn:
            drawn[k].add(kw[k])
    assert total >= 20000, total
    assert drawn["passing_only"] == {True, False} and drawn["het_only"] == {True, False} and len(drawn["distance"]) > 3 and len(drawn["min_passing"]) > 3
    short = {k: ref.COUNTS[k] for k in COUNTED if ref.COUNTS[k] < 20}
    assert not short, (short, dict(ref.COUNTS))


def test_count_word_and_the_rows_behind_it():
    recs, pairs = N.make_rows(N.seeded_rows(3, n=200, distance=10))
    kw = {"distance": 10, "passing_only": False}
    want = N.statement(recs[:120], pairs[:120], N.criteria_pair(**kw)[0])
    got = engine.nbhd_build(recs, pairs, N.criteria_pair(**kw)[1], count=120)
    N.assert_same(got, want, "count")


def test_refusals():
    recs, pairs = N.make_rows([(100, "A", "C", N.HET, 0), (101, "A", "C", N.HET, 0), (90, "A", "C", N.HET, 0), (80, "A", "C", N.HET, 0)])
    with pytest.raises(PiscesHipError) as e:
        engine.nbhd_build(recs, pairs)
    assert e.value.code == _abi.E_INVALID_ARG and e.value.n_out == (_abi.E_INVALID_ARG, 0, 2, 0, 0, 0) and e.value.message.endswith("not sorted by position at row 2")
    recs, pairs = N.make_rows([(100, "A", "C", N.HET, 0), (101, "AC", "A", N.HET, 0)])
    with pytest.raises(PiscesHipError) as e:
        engine.nbhd_build(recs, None)   # no candidate table
    assert e.value.code == _abi.E_INVALID_ARG and e.value.n_out == (_abi.E_INVALID_ARG, 1, 1, 0, 0, 0) and "without a candidate" in e.value.message
    full = engine.nbhd_build(recs, pairs)
    assert full["n_out"] == (1, 2, 5, 3, 1, 2)
    for short in ((0, 2, 5, 3), (1, 1, 5, 3), (1, 2, 4, 3), (1, 2, 5, 2)):
        with pytest.raises(PiscesHipError) as e:
            engine.nbhd_build(recs, pairs, capacities=short)
        assert e.value.code == _abi.E_BUFFER_TOO_SMALL and e.value.n_out == full["n_out"]
    crit = engine.nbhd_criteria()
    assert (crit.phasing_distance, crit.passing_variants_only, crit.het_variants_only, crit.min_passing_variants_in_nbhd) == (50, 1, 0, 0)
    from pisces_amd._native import lib
    import ctypes as C
    out = engine.nbhd_out(None, None, None, None, None, None, None, None, 0, 0, 0, 0)
    rows = engine.venn_rows(recs, len(recs))
    assert lib.pisces_hip_nbhd_build(C.byref(crit), C.byref(rows), None, 0, C.byref(out)) == _abi.E_INVALID_ARG
    assert b"null n_out" in lib.pisces_hip_last_error(None)
    assert lib.pisces_hip_nbhd_build(None, C.byref(rows), None, 0, C.byref(out)) == _abi.E_INVALID_ARG
    assert b"null criteria" in lib.pisces_hip_last_error(None)
