"""CoverageMethod.Exact without a device: the per-read decision (pisces_hip_exact_span_direction, the host form of csrc/exact_span.h, the
source exact_span_kernel compiles) against every ExecuteTest call of the reference's ExactCoverageCalculatorTests.cs
(tests/golden/exact_coverage_cases.json) and against the plain-Python statement tests/exact_ref.py, which is held to the same cases first;
and the statement's model of blocks, the look-forward window and retirement on hand-made reads."""
import collections
import json
import os
import random

import pytest

from pisces_amd import _abi, engine
from pisces_amd._native import PiscesHipError
from tests import exact_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N_SEEDED = 20000
DIRS = {"forward": R.FORWARD, "reverse": R.REVERSE, "stitched": R.STITCHED}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "exact_coverage_cases.json")) as f:
        return json.load(f)


def test_the_golden_file_holds_every_call_site(golden):
    assert golden["n_cases"] == len(golden["cases"]) == 53
    assert collections.Counter(c["category"] for c in golden["cases"]) == {"insertion": 18, "deletion": 17, "mnv": 18}


def test_statement_gives_the_reference_tests_directions(golden):
    for c in golden["cases"]:
        preceding, trailing = R.span_of(c["category"], c["position"], c["length"])
        got = R.direction(R.Summary(c["cs"], c["ce"], c["cigar"], c["directions"]), preceding, trailing)
        assert got == (None if c["expected"] is None else DIRS[c["expected"]]), c


def test_host_entry_gives_the_reference_tests_directions(golden):
    for c in golden["cases"]:
        preceding, trailing = R.span_of(c["category"], c["position"], c["length"])
        got = engine.exact_span_direction(c["cs"], c["ce"], c["cigar"], c["directions"], preceding, trailing, c["category"] == "insertion")
        assert got == (None if c["expected"] is None else DIRS[c["expected"]]), c


def test_first_and_last_operation_are_strict():
    """HasOperationAtOpIndex looks at the operation itself: 5M3I2S does not end in an insertion, 2S3I5M does not start with one"""
    for cigar, cs, ce, span, kept in (("5M3I", 6, 10, (10, 11), True), ("5M3I2S", 6, 10, (10, 11), False), ("5M3I2H", 6, 10, (10, 11), False),
                                      ("3I5M", 11, 15, (10, 11), True), ("2S3I5M", 11, 15, (10, 11), False)):
        n = sum(k for op, k in R.parse_cigar(cigar) if op in R.READ_SPAN)
        for runs in (f"{n}R", f"1F:{n - 1}S"):
            want = R.direction(R.Summary(cs, ce, cigar, runs), *span)
            assert (want is not None) == kept, (cigar, runs)
            assert engine.exact_span_direction(cs, ce, cigar, runs, *span) == want, (cigar, runs)


def test_position_map_takes_the_leading_clip_off_twice():
    """(:90) UpdatePositionMap(ClipAdjustedStart - GetPrefixClip()): 4S8M at Position 20 maps its aligned bases to 12 .. 19, not 20 .. 27"""
    s = R.Summary.of_read(20, "4S8M", [0] * 6 + [2] * 2 + [1] * 4)
    assert (s.cs, s.ce) == (16, 27)
    assert R.position_map(s.cs - R.prefix_clip(s.cigar), s.cigar) == [-2] * 4 + list(range(12, 20))
    # a deletion 17 > 20: preceding 17, trailing 21.  Through the shifted map: index 9 (position 17) and nothing at or behind 21 -> the bases
    # behind index 9 up to the read's end, R R.  From Position the indices would be none and 5, and the answer Forward.
    assert R.direction(s, 17, 21) == R.REVERSE
    assert engine.exact_span_direction(s.cs, s.ce, s.cigar, s.runs, 17, 21) == R.REVERSE


def test_both_indices_missing_is_the_references_exception():
    """A real read reaches it: several directions, a leading soft clip, and a deletion that starts in front of the shifted map and ends behind it"""
    s = R.Summary.of_read(100, "5S10M", [0] * 5 + [2] * 5 + [1] * 5)
    with pytest.raises(R.InvalidIndices):
        R.direction(s, 85, 100)
    with pytest.raises(PiscesHipError, match="Invalid indices"):
        engine.exact_span_direction(s.cs, s.ce, s.cigar, s.runs, 85, 100)
    with pytest.raises(PiscesHipError, match="longer than"):
        engine.exact_span_direction(6, 14, "9M", "2F:5S:3R", 10, 11)


# ---- seeded summaries: arbitrary CIGARs, 1-4 direction runs, spans at every relation to the read's ends ------------------------------------
def _random_cigar(rng):
    ops = []
    if rng.random() < 0.15:
        ops.append(("H", rng.randint(1, 4)))
    if rng.random() < 0.35:
        ops.append(("S", rng.randint(1, 6)))
    if rng.random() < 0.15:
        ops.append(("I", rng.randint(1, 4)))   # an insertion first (after the clips, or the read's strict first operation)
    body = rng.randint(1, 5)
    for k in range(body):
        ops.append((rng.choice("MMM=X"), rng.randint(1, 9)))
        if k + 1 < body:
            r = rng.random()
            if r < 0.3:
                ops.append(("I", rng.randint(1, 5)))
            elif r < 0.6:
                ops.append(("D", rng.randint(1, 6)))
            elif r < 0.7:
                ops.append(("N", rng.randint(1, 8)))
            elif r < 0.78:
                ops.append(("P", rng.randint(1, 3)))
    if rng.random() < 0.08:
        ops = [op for op in ops if op[0] not in "M=X"] or [("I", 3)]   # no aligned base at all
    if rng.random() < 0.15:
        ops.append(("I", rng.randint(1, 4)))   # an insertion last
    if rng.random() < 0.1:
        ops.append(("D", rng.randint(1, 4)))   # a deletion at the read's end / in front of the final clip
    if rng.random() < 0.35:
        ops.append(("S", rng.randint(1, 6)))
    if rng.random() < 0.15:
        ops.append(("H", rng.randint(1, 4)))
    return ops


def _random_runs(rng, n):
    k = min(rng.choice((1, 1, 2, 2, 3, 3, 3, 4)), max(n, 1))
    if n == 0:
        return [(rng.randrange(3), 0)]
    cuts = sorted(rng.sample(range(1, n), k - 1)) if k > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    runs, last = [], None
    for length in lens:
        d = rng.choice([x for x in range(3) if x != last])
        runs.append((d, length))
        last = d
    return runs


def _random_case(rng):
    cigar = _random_cigar(rng)
    position = rng.choice((1, 2, 7, 50, 1000, 2147480000)) + rng.randint(0, 5)
    n = sum(k for op, k in cigar if op in R.READ_SPAN)
    runs = _random_runs(rng, n)
    ref_span = sum(k for op, k in cigar if op in R.REF_SPAN)
    cs = position - R.prefix_clip(cigar)
    ce = position + ref_span - 1 + R.suffix_clip(cigar)
    if rng.random() < 0.1:   # the reference's mock hands summaries over as given: ends that no read would have
        cs += rng.randint(-3, 3)
        ce += rng.randint(-3, 3)
    map_start = cs - R.prefix_clip(cigar)
    anchors = (cs, ce, position, position + ref_span - 1, map_start, map_start + ref_span - 1, (cs + ce) // 2)
    preceding = rng.choice(anchors) + rng.randint(-3, 3)
    trailing = preceding + rng.choice((1, 1, 2, 3, 5, 9, 20, rng.choice(anchors) - preceding + rng.randint(-2, 2)))
    return R.Summary(cs, ce, cigar, runs), preceding, max(trailing, preceding)


def test_host_entry_equals_the_statement_on_seeded_summaries():
    rng = random.Random(20260119)
    seen = collections.Counter()
    outcomes = collections.Counter()
    for k in range(N_SEEDED):
        s, preceding, trailing = _random_case(rng)
        trace = []
        try:
            want = R.direction(s, preceding, trailing, trace)
        except R.InvalidIndices:
            want = "invalid"
        seen.update(trace)
        try:
            got = engine.exact_span_direction(s.cs, s.ce, s.cigar, s.runs, preceding, trailing, bool(k & 1))
        except PiscesHipError as e:
            assert "Invalid indices" in e.message, (e.message, s.cs, s.ce, s.cigar, s.runs, preceding, trailing)
            got = "invalid"
        assert got == want, (s.cs, s.ce, s.cigar, s.runs, preceding, trailing, trace)
        outcomes[want] += 1
    print("\nbranches of the per-read decision reached by", N_SEEDED, "seeded summaries:")
    for name in R.BRANCHES:
        print(f"  {name:48s} {seen[name]}")
    print("outcomes:", dict(outcomes))
    never = [name for name in R.BRANCHES if seen[name] == 0]
    assert not never, f"branches no seeded summary reached: {never}"
    assert not set(seen) - set(R.BRANCHES), set(seen) - set(R.BRANCHES)   # ("direction:adjacent-no-trailing" cannot be reached: see exact_ref.BRANCHES)
    assert all(outcomes[o] > 0 for o in (None, 0, 1, 2, "invalid"))


# ---- the statement's state manager ------------------------------------------------------------------------------------------------------
def test_summaries_live_in_the_block_of_their_clip_adjusted_end():
    st = R.ExactState(100)
    st.add_read(90, "8M5S", [0] * 13)          # aligned 90 .. 97, CE 102: block 2 exists because of the summary alone
    assert sorted(st.blocks) == [1, 2]
    assert st.counts(95, 96) == [1, 0, 0]
    st.done_processing(st.keys_to_flush(100))   # block 1 goes, the summary stays with block 2
    assert sorted(st.blocks) == [2] and st.counts(95, 96) == [1, 0, 0]
    st.done_processing(st.keys_to_flush(None))
    assert st.counts(95, 96) == [0, 0, 0]


def test_look_forward_window_is_twice_the_first_reads_length():
    st = R.ExactState(1000)
    st.add_read(10, "4M", [1] * 4)              # the first read: _readLength 4
    st.add_read(20, "30M", [0] * 30)            # CE 49
    assert st.counts(40, 41) == [1, 0, 0]       # 49 <= 41 + 8
    assert st.counts(39, 40) == [0, 0, 0]       # 49 >  40 + 8: the walk stops before the summary's position
    assert st.counts(11, 12) == [0, 1, 0]


def test_compute_fills_the_three_fields():
    st = R.ExactState(1000)
    for _ in range(3):
        st.add_read(5, "10M", [0] * 10)
    st.add_read(5, "10M", [0] * 4 + [2] * 3 + [1] * 3)
    assert st.compute("insertion", 9, 2, 1) == {"coverage_by_dir": [3, 0, 1], "total_coverage": 4, "reference_support": 3}
    assert st.compute("deletion", 6, 3, 9) == {"coverage_by_dir": [3, 0, 1], "total_coverage": 4, "reference_support": 0}
    assert st.compute("mnv", 12, 2, 0)["coverage_by_dir"] == [3, 1, 0]   # (the stitched read: the bases between positions 11 and 14 are R R)


def test_abi_constants():
    assert (_abi.COVERAGE_APPROXIMATE, _abi.COVERAGE_EXACT) == (0, 1)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pisces_hip.h")).read()
    assert "enum { PISCES_COVERAGE_APPROXIMATE = 0, PISCES_COVERAGE_EXACT = 1 };" in header
