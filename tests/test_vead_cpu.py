"""Scylla's read pass on the CPU: the plain-Python statement (tests/vead_ref.py, written from the reference's C#) reproduces the reference's
own test facts (tests/golden/vead_cases.json), and the host entries of the library (pisces_hip_vead_site_states,
pisces_hip_vead_neighborhood_info, pisces_hip_vead_groups: csrc/vead.h, the source the device compiles too) reproduce the statement — on
the golden cases, on seeded reads x site lists with every branch of the decision taken, and on the reference's chr21 Scylla BAM."""
import os
import random

import numpy as np
import pytest

from pisces_amd import _abi, engine
from pisces_amd._native import PiscesHipError
from tests import vead_cases as V
from tests import vead_ref as R

G = V.golden()
STATE_OF_RESULT = {R.THIS: R.ALT, R.DIFFERENT: R.OTHER, R.REFERENCE: R.REF, R.INSUFFICIENT: R.NONE}


def both(read, site_rows, min_q, min_sites=1):
    """(statement, host entry) for one read: (states or None, sites in range)"""
    position, cigar, bases, quals = read
    want, n, _ = R.read_states(min_q, position, cigar, bases, quals, V.sites_of(site_rows), min_sites)
    states, found = engine.vead_site_states(position, cigar, bases, quals, site_rows, engine.vead_options(min_base_call_quality=min_q))
    got = [int(s) for s in states] if found >= min_sites else None
    return (want, n), (got, found)


@pytest.mark.parametrize("case", G["finder_cases"], ids=lambda c: c["name"])
def test_finder_facts(case):
    """VeadFinderTests.cs: segment counts per type, lastPosInAlignment where the fact asserts it, and the print of every site"""
    read = V.golden_read(case)
    found, last = R.segments_of_read(case["min_q"], *read)
    assert {k: len(found[k]) for k in "MID"} == case["segments"]
    if "last_pos" in case:
        assert last == case["last_pos"]
    want, got = both(read, case["sites"], case["min_q"])
    assert want == got
    if case["expected"] is None:
        assert want[0] is None or not case["sites"]
        return
    for i, printed in enumerate(case["expected"]):
        if printed is not None:   # (the fact asserts only some sites)
            assert want[0][i] == V.state_of_print(case["sites"][i], printed), (i, printed)


@pytest.mark.parametrize("case", G["check_cases"], ids=lambda c: f"{c['family']}-{c['segment'][0]}-{c['segment'][1]}")
def test_check_variant_sequence_families(case):
    """CheckVariantSequenceForMatchInVariantSiteFromReadTest's four families: the statement's function directly, and the same question
    put to the host entry as a read whose one match segment is the fact's (a base N in the fact is a base N of the read)"""
    look, (p, alt) = R.Site(*case["look"]), case["segment"]
    assert R.check_match(look, R.Site(p, "R" * len(alt), alt)) == case["state"]
    read = (p, [("M", len(alt))], alt, [30] * len(alt))
    want, got = both(read, [case["look"]], 20, min_sites=0)
    assert want == got
    if look.pos >= p and look.pos <= p + len(alt):   # the site is in the read's range: the state is the fact's
        assert want[0] == R.canonical([look], [STATE_OF_RESULT[case["state"]]])


def one_neighbourhood(reads, site_rows, min_q=20):
    got = engine.vead_groups(V.batch_of(reads), site_rows, [(0, len(site_rows))], engine.vead_options(min_base_call_quality=min_q))
    V.assert_same(got, V.statement(reads, site_rows, [(0, len(site_rows))], min_q))
    return got


@pytest.mark.parametrize("case", G["get_veads"], ids=lambda c: c["name"])
def test_get_veads(case):
    """VeadSourceTests.GetVeads: which reads become groups, and the look-ahead it asserts (801 / 809)"""
    # CreateRead's qualityForAll is the read's MapQuality too: the MAPQ test belongs to whoever makes the batch
    reads = [(p, [("M", len(b))], b, [q] * len(b)) for p, b, q in case["reads"] if q >= case["min_map_quality"]]
    got = one_neighbourhood(reads, case["sites"], case["min_q"])
    assert int(got["info"]["last_with_look_ahead"][0]) == case["last_with_look_ahead"]
    assert [reads[r][0] for r in got["groups"]["first_read"]] == case["group_read_positions"]
    assert list(got["groups"]["n_veads"]) == case["n_veads"]
    assert engine.vead_neighborhood_info(case["sites"])[1] == case["last_with_look_ahead"]


@pytest.mark.parametrize("case", G["group_veads"], ids=lambda c: c["name"])
def test_group_veads(case):
    """VeadSourceTests.GroupVeads: the memberships in the Dictionary's enumeration order ({3, 5, 1, 1})"""
    reads = [(100, [("M", len(b))], b, [30] * len(b)) for b in case["reads"]]
    got = one_neighbourhood(reads, case["sites"])
    assert list(got["groups"]["n_veads"]) == case["memberships"]


def test_neighbourhood_filter_facts():
    """NbhdReadFilterTests.cs and VcfNeighborhoodTests.SetRangeOfInterestTests through the statement and the host entries"""
    F = G["filters"]
    for case in F["past"]:
        first, last, _, _ = R.neighborhood_bounds(V.sites_of(case["sites"]))
        assert engine.vead_neighborhood_info(case["sites"])[:2] == (first, last)
        for position, past in case["reads"]:
            assert (position > last) == past
            reads = [(position, [("M", 4)], "ACGT", [30] * 4)]
            assert int(one_neighbourhood(reads, case["sites"])["info"]["n_reads_used"][0]) == (0 if past or position + 4 - 1 < first else 1)
    for case in F["skip"]:
        first = R.neighborhood_bounds(V.sites_of(case["sites"]))[0]
        for position, skip in case["reads"]:
            assert (position + 4 - 1 < first) == skip
            reads = [(position, [("M", 4)], "ACGT", [30] * 4)]
            assert int(one_neighbourhood(reads, case["sites"])["info"]["n_reads_used"][0]) == (0 if skip else 1)
    for case in F["clipped"]:
        bounds = R.neighborhood_bounds(V.sites_of(case["sites"]))
        assert bounds[2:] == (case["soft_clip_end_before"], case["soft_clip_pos_after"])
        assert engine.vead_neighborhood_info(case["sites"]) == bounds
        for position, cigar, clipped in case["reads"]:
            reads = [(position, V.parse_cigar(cigar), "ACGT", [30] * 4)]
            assert int(one_neighbourhood(reads, case["sites"])["info"]["n_clipped_reads"][0]) == int(clipped)
    for case in F["range_of_interest"]:
        first, last, _, _ = engine.vead_neighborhood_info(case["sites"])
        assert (first, case["sites"][-1][0], last) == (case["first"], case["last_in_vcf"], case["last_with_look_ahead"])


FUZZ_READS = 20000
BRANCHES_WANTED = (["out of range", "no segment of the type", "gone past", "IDontKnow rescued to reference",
                    "deletion quality: after taken from the last base", "deletion quality: before taken from after"] +
                   [f"{kind}: {result}" for kind in "MID" for result in (R.THIS, R.REFERENCE, R.DIFFERENT, R.INSUFFICIENT)])


def test_host_entry_equals_statement_on_seeded_reads():
    """20 000 seeded reads x site lists: M I D S N = X H operations, qualities around the threshold, N bases, deletions first and last,
    insertions at the read's end, sites before / inside / straddling / behind every segment, A>A and co-located sites.  The statement counts
    its branches; none may stay cold."""
    rng = random.Random(20261021)
    R.BRANCHES.clear()
    for i in range(FUZZ_READS):
        force = (None, None, None, "D first", "D last", "I last")[i % 6]
        read = V.random_read(rng, force=force)
        min_q = rng.choice((0, 20, 20, 20, 21))
        rows = V.random_sites(rng, read, min_q, rng.randint(1, 8))
        min_sites = rng.choice((0, 1, 1, 2))
        want, got = both(read, rows, min_q, min_sites)
        assert want == got, (read, rows, min_q, min_sites)
    cold = [b for b in BRANCHES_WANTED if R.BRANCHES[b] == 0]
    assert not cold, (cold, dict(R.BRANCHES))


def test_groups_of_seeded_batches():
    """pisces_hip_vead_groups == the statement's groups over whole batches: overlapping neighbourhoods, soft clips, reads that are counted
    as clipped and then skipped, a neighbourhood no read reaches"""
    for seed in range(6):
        rng = random.Random(seed)
        reads = V.seeded_batch(seed, 300, start=1000, step=(0, 2), ops="MMMMMIDSSN=XH")
        rows = sorted(r for k in range(0, 300, 25) for r in V.random_sites(rng, reads[k], 20, 3))
        nbhd = V.chain(rows, 30) + [(0, min(5, len(rows))), (len(rows) - 1, len(rows))]
        rows = rows + [(5, "A", "C"), (100000, "A", "C")]
        nbhd += [(len(rows) - 2, len(rows) - 1), (len(rows) - 1, len(rows))]   # before every read, behind every read
        got = engine.vead_groups(V.batch_of(reads), rows, nbhd)
        V.assert_same(got, V.statement(reads, rows, nbhd), seed)
        assert got["info"]["n_clipped_reads"].sum() > 0 and len(got["groups"]) > len(nbhd)


def test_clipped_is_counted_before_the_skip_and_at_the_stopping_read():
    """VeadGroupSource.cs:56-66: the clip test comes first.  Site 10 A>C: SoftClipEndBeforeNbhd 9, FirstPositionOfInterest 10.  A 2M2S read
    at 8 ends at 9: clipped, then skipped.  A read of soft clip and insertion only, at LastPositionOfInterestWithLookAhead + 1, ends on the
    look-ahead position and is the read the scan stops at: still clip-tested."""
    rows = [(10, "A", "C")]
    reads = [(8, V.parse_cigar("2M2S"), "ACGT", [30] * 4), (12, V.parse_cigar("2I2S"), "ACGT", [30] * 4), (12, V.parse_cigar("4M"), "ACGT", [30] * 4)]
    got = one_neighbourhood(reads, rows)
    assert (int(got["info"]["n_clipped_reads"][0]), int(got["info"]["n_reads_used"][0])) == (2, 0)
    assert R.neighborhood_bounds(V.sites_of(rows)) == (10, 11, 9, 11)


@pytest.fixture(scope="module")
def chr21():
    z = np.load(os.path.join(V.GOLDEN, "bam_scylla_chr21.npz"))
    rows = [(int(p), str(r), str(a)) for p, r, a in zip(z["vcf_position"], z["vcf_ref"], z["vcf_alt"])]
    return z, rows


def test_chr21_scylla_bam(chr21):
    """The reference's own Scylla input: 1031 chr21 alignments, the variant rows of its gVCF chained at distance 50 (one neighbourhood of
    well over 32 sites: a one-word key is not enough), and each row as a neighbourhood of its own"""
    z, rows = chr21
    reads = V.reads_of(z)
    nbhd = V.chain(rows, 50)
    assert max(e - b for b, e in nbhd) > 32
    nbhd += [(i, i + 1) for i in range(len(rows))]
    got = engine.vead_groups(z, rows, nbhd)
    V.assert_same(got, V.statement(reads, rows, nbhd))
    assert len(got["groups"]) > 100 and got["info"]["n_clipped_reads"].max() > 0


def refused(code, word, *args, **kw):
    with pytest.raises(PiscesHipError) as e:
        engine.vead_groups(*args, **kw)
    assert e.value.code == code and word in e.value.message, e.value
    return e.value


def test_refusals():
    reads = V.seeded_batch(1, 5)
    batch = V.batch_of(reads)
    rows = [(1000, "A", "C"), (1002, "AC", "A")]
    unsorted = dict(batch, position=np.array([1000, 1001, 1000, 1003, 1004], dtype=np.int32))
    e = refused(_abi.E_INVALID_ARG, "not sorted by position at read 2", unsorted, rows, [(0, 2)])
    assert e.n_out == (_abi.E_INVALID_ARG, 0, 2)
    many = [(1000 + i, "A", "C") for i in range(_abi.VEAD_MAX_SITES + 1)]
    refused(_abi.E_UNSUPPORTED, "PISCES_VEAD_MAX_SITES", batch, many, [(0, len(many))])
    engine.vead_groups(batch, many, [(0, _abi.VEAD_MAX_SITES)])
    refused(_abi.E_INVALID_ARG, "is empty", batch, rows, [(1, 1)])
    refused(_abi.E_INVALID_ARG, "outside the site list", batch, rows, [(0, 3)])
    sites, alleles = engine.vead_sites(rows)
    sites["alt_len"][1] = 0
    refused(_abi.E_INVALID_ARG, "below 1", batch, (sites, alleles), [(0, 2)])
    e = refused(_abi.E_BUFFER_TOO_SMALL, "do not fit", batch, [(reads[0][0], "A", "C")], [(0, 1)], capacities=(0, 0))
    assert e.n_out[0] >= 1 and e.n_out[1] == e.n_out[0] and e.n_out[2] == 0
    assert _abi.ABI_VERSION == 9 and _abi.VEAD_MAX_SITES >= 256
