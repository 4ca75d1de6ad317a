"""The amplicon-bias filter without a device: the decision (pisces_hip_amplicon_bias, the host form of csrc/amplicon_bias.h) against the
reference's own unit tests (tests/golden/amplicon_bias_cases.json) and against the plain-Python statement tests/amplicon_ref.py, which is
held to the same cases first; and the AB filter name in the VCF writer."""
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import amplicon_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILTER_STRAND_BIAS, FILTER_AMPLICON_BIAS, FILTER_RMXN = 0, 2, 9
N_SEEDED = 20000


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "amplicon_bias_cases.json")) as f:
        return json.load(f)


def both_ways_round(case):
    """The case as it stands and as ReverseAmpliconData hands it over"""
    yield case["support"], case["coverage"]
    yield dict(reversed(list(case["support"].items()))), dict(reversed(list(case["coverage"].items())))


def aligned(support, coverage):
    """What crosses the C boundary: one entry per amplicon of the coverage list, the support found under its name"""
    return [support.get(name, 0) for name in coverage], list(coverage.values())


def library_answer(support, coverage, threshold):
    """pisces_hip_amplicon_bias's three answers in the reference's terms.  Aligned by name, a support list without counts and an empty one are
    the same arrays: the library answers -1 (nothing to filter on) where the reference has a result that says False."""
    sup, cov = aligned(support, coverage)
    detected, chance = engine.amplicon_bias(sup, cov, threshold)
    if detected is None:
        assert len(cov) < 2 or not any(sup), (support, coverage)   # -1 exactly where the header says
        return None, None
    assert len(cov) >= 2 and any(sup), (support, coverage)
    return detected, chance


def seeded_sets(seed=20180417, n=N_SEEDED):
    """(support, coverage, threshold) of 2-6 amplicons: one variant frequency for the locus, every amplicon sampling it at its own depth,
    some amplicons depleted (the artefact the filter looks for), some without coverage; thresholds around the option's usual values."""
    rng = np.random.default_rng(seed)
    thresholds = (0.01, 0.001, 0.05, 0.2, 0.5)
    for _ in range(n):
        k = int(rng.integers(2, 7))
        vf = float(rng.choice((0.005, 0.01, 0.02, 0.05, 0.08, 0.1, 0.12, 0.3)))
        coverage = [int(c) for c in rng.choice((0, 30, 200, 1000, 5000), size=k) * rng.uniform(0.5, 1.5, size=k)]
        keep = rng.choice((0.0, 0.3, 0.6, 0.8, 1.0, 1.1), size=k)
        support = [int(min(c, rng.poisson(c * vf * f))) for c, f in zip(coverage, keep)]
        yield support, coverage, float(rng.choice(thresholds))


def test_python_statement_reproduces_the_reference_unit_tests(golden):
    assert len(golden["cases"]) == 1000 + 20 + 1 + 3 + 9
    for case in golden["cases"]:
        for support, coverage in both_ways_round(case):
            assert R.bias_detected(support, coverage, golden["threshold"]) == case["expected"], case


def test_library_reproduces_the_reference_unit_tests(golden):
    for case in golden["cases"]:
        for support, coverage in both_ways_round(case):
            detected, _ = library_answer(support, coverage, golden["threshold"])
            sup, cov = aligned(support, coverage)
            if case["expected"] is None or not any(sup):
                # the reference's null result, and its False for a support list whose names hold no count or match no coverage name
                # (C, D against A, B; "no support anywhere"): aligned by name these are one input, and the entry answers -1 for it
                assert case["expected"] in (None, False) and detected is None, case
            else:
                assert detected is case["expected"], case


def test_library_agrees_with_the_python_statement_on_seeded_sets():
    n = n_poisson = n_detected = 0
    for support, coverage, threshold in seeded_sets():
        names = [f"amp{i}" for i in range(len(coverage))]
        sup_by, cov_by = {a: s for a, s in zip(names, support) if s > 0}, dict(zip(names, coverage))
        want, want_chance = R.bias_detected(sup_by, cov_by, threshold), R.chances(sup_by, cov_by)
        detected, chance = library_answer(sup_by, cov_by, threshold)
        assert detected == want, (support, coverage, threshold)
        if want is not None:
            np.testing.assert_allclose(chance, want_chance, rtol=1e-12, atol=0.0, err_msg=str((support, coverage)))
            n_poisson += sum(0.0 < p < 1.0 for p in want_chance)
            n_detected += bool(want)
        n += 1
    assert n == N_SEEDED
    # the sets reach the Poisson tail and both answers often enough to mean something
    assert n_poisson > N_SEEDED // 4 and N_SEEDED // 10 < n_detected < N_SEEDED * 9 // 10, (n_poisson, n_detected)


def test_no_case_sits_on_its_threshold(golden):
    """From the Python statement alone: no p_i of any case the tests above decide lies within 1e-6 (relative) of its threshold, so a last-digit
    difference between two Poisson.Cdf implementations cannot change an expected answer.  None left out."""
    for case in golden["cases"]:
        assert R.margin_to_threshold(case["support"], case["coverage"], golden["threshold"]) > 1e-6, case
    for support, coverage, threshold in seeded_sets():
        names = [f"amp{i}" for i in range(len(coverage))]
        sup_by = {a: s for a, s in zip(names, support) if s > 0}
        assert R.margin_to_threshold(sup_by, dict(zip(names, coverage)), threshold) > 1e-6, (support, coverage, threshold)


def test_threshold_is_compared_as_the_float_it_is():
    # Poisson.Cdf(0, 5) = exp(-5) = 0.006737946999...: a threshold one float above it fails the amplicon, the float at or below does not
    p = R.chances({"a": 50}, {"a": 1000, "b": 100})[1]
    assert abs(p - np.exp(-5.0)) < 1e-12
    above = np.nextafter(np.float32(p), np.float32(1.0))
    below = np.nextafter(above, np.float32(0.0), dtype=np.float32)
    assert float(below) <= p < float(above)
    for threshold, want in ((above, True), (np.nextafter(below, np.float32(0.0)), False)):
        assert R.bias_detected({"a": 50}, {"a": 1000, "b": 100}, threshold) is want
        assert engine.amplicon_bias([50, 0], [1000, 100], threshold)[0] is want


def test_no_result_and_degenerate_arguments():
    assert engine.amplicon_bias([7], [100], 0.01) == (None, None)              # one amplicon: no bias to detect
    assert engine.amplicon_bias([], [], 0.01) == (None, None)
    assert engine.amplicon_bias([0, 0, 0], [500, 500, 500], 0.01) == (None, None)   # nobody tagged supports the allele
    assert engine.lib.pisces_hip_amplicon_bias(None, None, 2, 0.01, None) == -1
    detected, chance = engine.amplicon_bias([20, 0, 0], [200, 0, 200], 0.0)     # threshold 0: tracked, nothing can fail
    assert detected is False and chance[1] == 1.0 and 0.0 < chance[2] < 1e-8
    # more amplicons than the store's six slots: the calculator has no limit of its own
    detected, chance = engine.amplicon_bias([30] * 7 + [0], [300] * 8, 0.01)
    assert detected is True and list(chance[:7]) == [1.0] * 7 and chance[7] < 1e-12


def _snv(filters):
    r = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)
    r["position"], r["total_coverage"], r["allele_support"], r["reference_support"] = 567, 400, 20, 380
    r["variant_qscore"], r["genotype_qscore"], r["strand_bias_score"] = 100, 100, 1.0
    r["filter_bits"] = sum(1 << f for f in filters)
    r["info"] = 2 | (_abi.CAT_SNV << 4) | (0 << 7) | (3 << 10)   # 0/1, A>T
    return r


def test_vcf_names_the_filter_in_processor_order():
    # AlleleProcessor.ApplyFilters adds AmpliconBias behind StrandBias and before the repeat filters (AlleleProcessor.cs:45-63)
    text = engine.format_vcf("chr1", _snv((FILTER_RMXN, FILTER_AMPLICON_BIAS, FILTER_STRAND_BIAS)))
    assert text.split("\t")[6] == "SB;AB;R5x9"


def test_vcf_prints_the_filter_alone():
    # VcfFormatter.MapFilter: FilterType.AmpliconBias -> "AB" (VcfFormatter.cs:22,155-156)
    text = engine.format_vcf("chr1", _snv((FILTER_AMPLICON_BIAS,)))
    assert text.split("\t")[6] == "AB"


def test_python_statement_of_the_counts_on_hand_worked_reads():
    """AddAlleleCounts' rule for AddAmpliconCount (RegionStateManager.cs:179-189), worked by hand: aligned A/C/G/T bases at or above the minimum
    quality count under their read's name; soft clips, inserted bases, deleted positions, N and low-quality bases and untagged reads do not."""
    q = lambda s: bytes(30 if c == "+" else 5 for c in s)
    reads = [
        dict(pos=100, cigar=[("S", 2), ("M", 4)], seq="TTACGT", quals=q("++++++")),               # 100 A, 101 C, 102 G, 103 T
        dict(pos=101, cigar=[("M", 2), ("I", 1), ("M", 1)], seq="CGAT", quals=q("++++")),         # 101 C, 102 G, (A inserted), 103 T
        dict(pos=100, cigar=[("M", 1), ("D", 2), ("M", 1)], seq="AT", quals=q("++")),             # 100 A, 101-102 deleted, 103 T
        dict(pos=100, cigar=[("M", 4)], seq="ANGA", quals=q("+++-"), reverse=True),              # 100 A, 101 N, 102 G, 103 low quality
        dict(pos=100, cigar=[("M", 4)], seq="ACGT", quals=q("++++")),                             # untagged
    ]
    coverage, support = R.amplicon_counts(reads, ["x", "y", "x", "y", None])
    assert coverage == {100: {"x": 2, "y": 1}, 101: {"x": 1, "y": 1}, 102: {"x": 1, "y": 2}, 103: {"x": 2, "y": 1}}
    assert support[100] == {"A": {"x": 2, "y": 1}} and support[102] == {"G": {"x": 1, "y": 2}} and support[103] == {"T": {"x": 2, "y": 1}}
    # the SNV 103 T>A of the low-quality base has no tagged support; an SNV's lists feed the decision as they are
    assert R.bias_detected(support[103].get("A", {}), coverage[103], 0.01) is None
    # the seventh name on one position is the reference's IndexOutOfRangeException; six are fine
    one = lambda name: dict(pos=200, cigar=[("M", 1)], seq="A", quals=q("+"))
    assert len(R.amplicon_counts([one(i) for i in range(6)], list(range(6)))[0][200]) == 6
    with pytest.raises(R.TooManyAmplicons) as e:
        R.amplicon_counts([one(i) for i in range(7)], list(range(7)))
    assert e.value.position == 200


def test_no_decision_of_the_gpu_scenarios_sits_on_its_threshold():
    """The same margin for every SNV the scenarios of tests/test_amplicon_gpu.py can call: every (position, base) with tagged or untagged
    support, none left out; and the planted loci decide as the scenario says."""
    from tests import amplicon_cases as S
    for make in (S.filter_scenario, S.counts_scenario):
        ref, reads, ids = make()
        coverage, support = R.amplicon_counts(reads, S.names_of(ids))
        for position, by_base in support.items():
            for base, sup in by_base.items():
                if base != chr(ref[position - 1]):
                    assert R.margin_to_threshold(sup, coverage[position], S.THRESHOLD) > 1e-6, (position, base)
    ref, reads, ids = S.filter_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids))
    for position, (_, want) in S.PLANTED.items():
        if want == "no SNV row":
            continue
        alt = S.OTHER[chr(ref[position - 1])]
        assert R.bias_detected(support.get(position, {}).get(alt, {}), coverage[position], S.THRESHOLD) is want, position


def test_the_haploid_scenario_decides_as_it_says_and_off_its_threshold():
    from tests import amplicon_cases as S
    ref, reads, ids = S.haploid_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids))
    assert sorted(p for p, by in support.items() if set(by) != {chr(ref[p - 1])}) == sorted(S.HAPLOID_PLANTED)
    for position, want in S.HAPLOID_PLANTED.items():
        alt = S.OTHER[chr(ref[position - 1])]
        assert sum(support[position][alt].values()) > 0.8 * sum(coverage[position].values())     # the locus' one allele for the haploid genotyper
        assert R.bias_detected(support[position][alt], coverage[position], S.THRESHOLD) is want, position
        assert R.margin_to_threshold(support[position][alt], coverage[position], S.THRESHOLD) > 1e-6, position


# ---- the seeded generators of the device fuzz (tests/amplicon_cases.py): what they promise, from the data and the Python statement alone ----

_planted_cache = {}


def planted(seed, threshold):
    """(scenario, coverage, support) of a planted seed, made once"""
    from tests import amplicon_cases as S
    if (seed, threshold) not in _planted_cache:
        sc = S.planted_scenario(seed, threshold)
        _planted_cache[seed, threshold] = (sc,) + R.amplicon_counts(sc["reads"], S.names_of(sc["ids"]))
    return _planted_cache[seed, threshold]


def test_no_seed_of_the_generators_reaches_a_seventh_amplicon():
    """R.amplicon_counts raises TooManyAmplicons on a seventh id: it must not, for every listed seed, in every state the device tests
    bring a store to (the reads alone, with the batch that straddles the floor, the fresh batch alone; the all-tagged exotic variant)."""
    from tests import amplicon_cases as S
    for seed in S.TAGGED_SEEDS:
        for kw in ({}, dict(exotic=True, tag_all=True)):
            case = S.lifecycle_case(seed, **kw)
            text = lambda reads: [dict(r, seq=bytes(r["seq"]).decode("latin-1")) for r in reads]
            R.amplicon_counts(text(case["reads"] + case["ahead"][0]), S.names_of(case["ids"] + case["ahead"][1]))
            R.amplicon_counts(text(case["fresh"][0]), S.names_of(case["fresh"][1]))
    for seed, threshold in S.PLANTED_SEEDS:
        planted(seed, threshold)


def test_random_tagged_reads_contain_what_they_promise():
    from tests import amplicon_cases as S
    for seed in S.TAGGED_SEEDS:
        reads, ids = S.random_tagged_reads(seed)
        assert len(reads) == 614 and len(ids) == len(reads)
        ops = [set(op for op, _ in r["cigar"]) for r in reads]
        for op in "MIDSNHP=X":
            assert any(op in o for o in ops), (seed, op)
        assert any(r["cigar"][-1][0] == "D" for r in reads) and any(r["cigar"][0][0] == "D" for r in reads)   # terminal deletions
        assert any(b"N" in r["seq"] for r in reads) and {10, 25, 37, 200} <= set(q for r in reads for q in r["quals"])
        ordinary = [r for r in reads if S.ref_span(r) <= 0xFFFF]
        assert len(reads) - len(ordinary) == 6 and max(S.ref_span(r) for r in ordinary) < S.WINDOW
        assert sum(r["pos"] == 1 for r in reads) == 4
        assert sum(r["pos"] + S.ref_span(r) - 1 == S.FUZZ_REF_LENGTH for r in reads) == 5 and all(r["pos"] + S.ref_span(r) - 1 <= S.FUZZ_REF_LENGTH for r in reads)
        untagged = sum(i == -1 for i in ids)
        assert len(ids) // 9 < untagged < len(ids) // 5 and min(ids) == -1
        assert {0, 0x7FFFFFFF} <= set(ids)
        coverage, _ = R.amplicon_counts(reads, S.names_of(ids))
        assert {len(v) for v in coverage.values()} == {1, 2, 3, 4, 5, 6}, seed
        assert 1 in coverage and S.FUZZ_REF_LENGTH in coverage
        # tile edges and a block edge inside the range, and reads on both sides of them
        assert all(p in coverage for p in (1000, 1001, 1064, 1065, 1128, 1129))
        # every read tagged: the variant whose counts are held to the caller's own
        assert min(S.random_tagged_reads(seed, exotic=True, tag_all=True)[1]) >= 0


def test_no_decision_of_the_planted_scenarios_sits_on_its_threshold():
    """The margin of test_no_case_sits_on_its_threshold for every (position, base) with tagged or untagged support in every planted
    scenario, none left out (a seed that puts one inside the margin is replaced in the list)."""
    from tests import amplicon_cases as S
    assert sorted(t for _, t in S.PLANTED_SEEDS) == sorted(S.PLANTED_THRESHOLDS)
    for seed, threshold in S.PLANTED_SEEDS:
        sc, coverage, support = planted(seed, threshold)
        total = R.amplicon_counts(sc["reads"], [0] * len(sc["reads"]))[1]
        n = 0
        for position, by_base in total.items():
            for base in by_base:
                if base != chr(sc["ref"][position - 1]):
                    n += 1
                    assert R.margin_to_threshold(support.get(position, {}).get(base, {}), coverage.get(position, {}), threshold) > 1e-6, (seed, position, base)
        assert n >= 80, (seed, n)


def test_planted_scenarios_reach_every_answer_at_every_number_of_amplicons():
    """Over the listed seeds the statement decides the planted alleles 185 times True, 153 times False and 143 times None (asked: 40 / 40 / 10);
    by the number of amplicons at the locus, True: {2: 25, 3: 29, 4: 55, 5: 36, 6: 40}, False: {2: 44, 3: 41, 4: 47, 5: 9, 6: 12}.
    The loci hold position 1, the reference's last base, first / last / last-but-one positions of tiles, a block's first position, loci
    with two alternative bases and loci whose carriers have no tag; every region size 1..6 occurs in every scenario."""
    from tests import amplicon_cases as S
    counts = {True: {}, False: {}, None: {}}
    kinds = set()
    for seed, threshold in S.PLANTED_SEEDS:
        sc, coverage, support = planted(seed, threshold)
        assert 4000 <= len(sc["reads"]) <= 8000 and all(S.ref_span(r) == 100 for r in sc["reads"])
        assert {v["k"] for v in sc["loci"].values()} == {1, 2, 3, 4, 5, 6}
        positions = sorted(sc["loci"])
        assert len(positions) >= 70 and min(b - a for a, b in zip(positions, positions[1:])) >= 7
        assert 1 in sc["loci"] and len(sc["ref"]) in sc["loci"] and 1001 in sc["loci"]
        for position, locus in sc["loci"].items():
            k = len(coverage[position])
            assert k == locus["k"], (seed, position)
            kinds.add(("tile", (position - 1) % 1000 % 64))
            kinds.add(("alts", len(locus["alts"])))
            kinds.add(("untagged", locus["untagged"]))
            for alt in locus["alts"]:
                answer = R.bias_detected(support.get(position, {}).get(alt, {}), coverage[position], threshold)
                assert not (locus["untagged"] or k == 1) or answer is None
                counts[answer][k] = counts[answer].get(k, 0) + 1
    assert {("tile", 0), ("tile", 62), ("tile", 63), ("alts", 2), ("untagged", True)} <= kinds
    n = {answer: sum(by_k.values()) for answer, by_k in counts.items()}
    assert n[True] >= 40 and n[False] >= 40 and n[None] >= 10, n
    assert set(counts[True]) == {2, 3, 4, 5, 6} and set(counts[False]) == {2, 3, 4, 5, 6}, counts
    assert (n[True], n[False], n[None]) == (185, 153, 143), n     # the docstring's figures


def test_decision_does_not_depend_on_the_order_of_the_amplicons():
    """The device claims a locus' slots in arrival order, so amplicon::bias sees the amplicons in an order that differs from run to run
    (amplicon_bias.h: no decision depends on it).  On the host: the same decision and the same multiset of chances for the arrays as
    drawn, reversed and under three seeded permutations."""
    rng = np.random.default_rng(20260101)
    n_decided = 0
    for support, coverage, threshold in seeded_sets():
        detected, chance = engine.amplicon_bias(support, coverage, threshold)
        k = len(coverage)
        for order in [np.arange(k)[::-1]] + [rng.permutation(k) for _ in range(3)]:
            again, chance_again = engine.amplicon_bias([support[i] for i in order], [coverage[i] for i in order], threshold)
            assert again is detected, (support, coverage, threshold, list(order))
            if detected is not None:
                assert sorted(chance_again) == sorted(chance), (support, coverage, threshold, list(order))
                assert [chance_again[j] for j in np.argsort(order)] == list(chance)
        n_decided += detected is not None
    assert n_decided > N_SEEDED // 2
