"""The amplicon-bias filter on the device (amplicon_kernels.hip.h): per-amplicon counts from the read store against the plain-Python
statement (tests/amplicon_ref.py), the filter bit of a flush against its decision, through every route a batch and a flush can take, the
six-slot limit, the refusals, and that a handle without the filter is untouched.  Scenarios: tests/amplicon_cases.py."""
import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import amplicon_cases as S
from tests import amplicon_ref as R
from tests.test_read_store import env, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
AB = 1 << 2
BASE_OF_TYPE = "AGCT"
APPENDED = {"PISCES_HIP_STORE_DIRECT_BYTES": 1 << 40, "PISCES_HIP_STORE_SEAL_BYTES": 1 << 40}


@pytest.fixture(scope="module")
def filter_case():
    ref, reads, ids = S.filter_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids))
    return ref, reads, ids, coverage, support


@pytest.fixture(scope="module")
def counts_case():
    ref, reads, ids = S.counts_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids))
    total = R.amplicon_counts(reads, [0] * len(reads))[1]
    untagged = R.amplicon_counts(reads, [0 if i < 0 else None for i in ids])[1]
    return ref, reads, ids, coverage, support, total, untagged


def caller(ref, threshold=None, **cfg):
    c = engine.HipVariantCaller(_abi.default_config(**cfg), device=0)
    c.SetReference(ref)
    if threshold is not None:
        c.SetAmpliconBiasFilter(threshold)
    return c


def check_counts(c, lo, hi, coverage, support, untagged):
    ids, cov, sup = c.GetCoverageByAmplicon(lo, hi - lo + 1)
    folded = c.GetCounts(lo, hi - lo + 1).sum(axis=(2, 3))   # [n][AlleleType]
    for k, p in enumerate(range(lo, hi + 1)):
        want = sorted(coverage.get(p, {}).items())
        assert [int(x) for x in ids[k]] == [a for a, _ in want] + [-1] * (6 - len(want)), p
        assert [int(x) for x in cov[k]] == [n for _, n in want] + [0] * (6 - len(want)), p
        for b, base in enumerate("ACGT"):
            by = support.get(p, {}).get(base, {})
            assert [int(x) for x in sup[k, b]] == [by.get(a, 0) for a, _ in want] + [0] * (6 - len(want)), (p, base)
            # tagged support + the untagged reads' share = the allele count the caller itself uses
            assert int(sup[k, b].sum()) + sum(untagged.get(p, {}).get(base, {}).values()) == int(folded[k, BASE_OF_TYPE.index(base)]), (p, base)


def test_counts_match_the_python_statement_across_tile_and_block_edges(torch_cuda, counts_case):
    ref, reads, ids, coverage, support, total, untagged = counts_case
    with caller(ref, S.THRESHOLD) as c:
        c.AddAlleleCounts(reads, amplicon_ids=ids)
        check_counts(c, 930, 1100, coverage, support, untagged)
        rows = c.Call(1000)
        assert len(rows) and rows["position"].max() <= 1000
        check_counts(c, 1001, 1100, coverage, support, untagged)   # the floor has moved: the positions still held
        c.Call()


def test_counts_above_the_row_codes_quality_range(torch_cuda):
    """A threshold above 127 does not fit the row codes' low-quality bit: the kernel reads the qualities there, so a base of quality 128
    under a threshold of 130 counts for no amplicon, exactly as the caller's own counts drop it."""
    ref, reads, ids, min_bq = S.high_threshold_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids), min_base_call_quality=min_bq)
    assert R.amplicon_counts(reads, S.names_of(ids), min_base_call_quality=127)[0] != coverage    # the scenario has such bases
    with caller(ref, S.THRESHOLD, min_base_call_quality=min_bq) as c:
        c.AddAlleleCounts(reads, amplicon_ids=ids)
        check_counts(c, 940, 1060, coverage, support, {})


def expected_bits(rows, ref, coverage, support):
    want = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        if ((int(r["info"]) >> 4) & 7) != _abi.CAT_SNV or r["allele_support"] <= 0:
            continue
        p, alt = int(r["position"]), BASE_OF_TYPE[(int(r["info"]) >> 10) & 7]
        want[i] = R.bias_detected(support.get(p, {}).get(alt, {}), coverage.get(p, {}), S.THRESHOLD) is True
    return want


def assert_only_the_bit_differs(rows, plain, want):
    assert len(rows) == len(plain)
    a, b = rows.copy(), plain.copy()
    got = (a["filter_bits"] & AB) != 0
    assert not ((b["filter_bits"] & AB) != 0).any()
    a["filter_bits"] &= ~np.uint16(AB)
    assert a.tobytes() == b.tobytes()
    assert (got == want).all(), (rows["position"][got != want], got[got != want])


def run(route, ref, reads, ids, threshold, **cfg):
    with caller(ref, threshold, **cfg) as c:
        if route == "device":
            c.AddDeviceReads(reads, amplicon_ids=ids if threshold is not None else None)
            return c.CallView().copy()
        if route == "appended":
            for i in range(0, len(reads), 50):
                c.AddAlleleCounts(reads[i:i + 50], amplicon_ids=ids[i:i + 50] if threshold is not None else None)
            return np.concatenate([c.Call(199), c.Call()])
        c.AddAlleleCounts(reads, amplicon_ids=ids if threshold is not None else None)
        if route == "begin_end":
            c.CallBegin()
            return c.CallEnd()
        if route == "small_buffer":
            return c.Call(capacity=1)
        return c.Call()


def test_filter_bit_equals_the_python_decision_and_nothing_else_changes(torch_cuda, filter_case):
    ref, reads, ids, coverage, support = filter_case
    rows = run("plain", ref, reads, ids, S.THRESHOLD)
    plain = run("plain", ref, reads, ids, None)
    want = expected_bits(rows, ref, coverage, support)
    assert_only_the_bit_differs(rows, plain, want)
    flagged = {int(p) for p in rows["position"][(rows["filter_bits"] & AB) != 0]}
    assert flagged == {120, 125}
    snv = lambda p: [r for r in rows if r["position"] == p and ((int(r["info"]) >> 4) & 7) == _abi.CAT_SNV]
    for p in (120, 125, 140, 160, 230):
        assert len(snv(p)) == 1, p          # every planted SNV is called, so the three unflagged ones are decisions, not absences
    dels = [r for r in rows if ((int(r["info"]) >> 4) & 7) == _abi.CAT_DELETION]
    assert dels and not any(int(r["filter_bits"]) & AB for r in dels)


@pytest.mark.parametrize("route,cfg,environment", [
    ("appended", {}, APPENDED),
    ("device", {}, {}),
    ("begin_end", {}, {}),
    ("plain", {"ploidy": _abi.PLOIDY_DIPLOID}, {}),
    ("plain", {"noise_model": 1}, {}),
    ("plain", {"strand_bias_model": _abi.SB_DIPLOID}, {}),
    ("small_buffer", {}, {}),
], ids=["appended batches, two flushes", "device reads + flush_view", "flush_begin / flush_end", "DiploidByThresholding", "NoiseModel.Window",
        "Diploid strand-bias model", "too-small buffer first"])
def test_the_same_scenario_through_every_route(torch_cuda, filter_case, route, cfg, environment):
    ref, reads, ids, coverage, support = filter_case
    with env(**environment):
        rows = run(route, ref, reads, ids, S.THRESHOLD, **cfg)
        plain = run(route, ref, reads, ids, None, **cfg)
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, ref, coverage, support))
    flagged = {int(p) for p in rows["position"][(rows["filter_bits"] & AB) != 0]}
    # (whatever the diploid genotyper does with the 5 % allele at 120, the het call at 125 keeps its bit)
    assert 125 in flagged and flagged <= {120, 125} and (cfg.get("ploidy") or flagged == {120, 125})


def test_a_seventh_amplicon_at_one_position_is_an_error_of_the_flush(torch_cuda):
    ref = S.reference()
    # (an SNV every read carries: the pass counts in tiles that hold a supported SNV row, the others leave early)
    reads = [S._read(ref, 50, [("M", 10)], edits={55: S.OTHER[chr(ref[54])]}) for _ in range(70)]
    with caller(ref, S.THRESHOLD) as c:
        c.AddAlleleCounts(reads, amplicon_ids=[10 + i % 6 for i in range(70)])
        assert len(c.Call())
    with caller(ref, S.THRESHOLD) as c:
        c.AddAlleleCounts(reads, amplicon_ids=[10 + i % 7 for i in range(70)])
        with pytest.raises(engine.PiscesHipError) as e:
            c.Call()
        assert e.value.code == _abi.E_INVALID_ARG and "more than 6 amplicons" in e.value.message and "position 50)" in e.value.message
        assert int(c.GetCounts(50, 1).sum()) == 70     # the blocks stay held


def test_refusals_state_and_inertness(torch_cuda, filter_case):
    ref, reads, ids, coverage, support = filter_case

    def refused(code, f):
        with pytest.raises(engine.PiscesHipError) as e:
            f()
        assert e.value.code == code and e.value.message, e.value
    for cfg in ({"call_mnvs": 1}, {"collapse_freq_threshold": 0.1}, {"collapse_freq_ratio_threshold": 1.0}):
        with caller(ref, **cfg) as c:
            refused(_abi.E_UNSUPPORTED, lambda: c.SetAmpliconBiasFilter(S.THRESHOLD))
    with caller(ref) as c:
        c.SetForcedAlleles([(30, chr(ref[29]), S.OTHER[chr(ref[29])])])
        refused(_abi.E_UNSUPPORTED, lambda: c.SetAmpliconBiasFilter(S.THRESHOLD))
    with env(PISCES_HIP_READ_PATH="log"):
        with caller(ref) as c:
            refused(_abi.E_UNSUPPORTED, lambda: c.SetAmpliconBiasFilter(S.THRESHOLD))
    with caller(ref, S.THRESHOLD) as c:
        refused(_abi.E_UNSUPPORTED, lambda: c.SetForcedAlleles([(30, chr(ref[29]), S.OTHER[chr(ref[29])])]))
        refused(_abi.E_UNSUPPORTED, c.AddDecodedReads)
        refused(_abi.E_UNSUPPORTED, lambda: c.AddObservations(np.array([5], dtype=np.int32), np.array([0], dtype=np.uint32)))
        refused(_abi.E_INVALID_ARG, lambda: c.AddAlleleCounts(reads[:3], amplicon_ids=[1, -2, 1]))
        refused(_abi.E_INVALID_ARG, lambda: c.AddDeviceReads(reads[:3], amplicon_ids=[1, 1, -2]))     # the same check, made on the device
        assert int(c.GetCounts(100, 100).sum()) == 0   # the refused batch left nothing
        c.AddAlleleCounts(reads[:3])                    # the plain add still works: its reads carry -1
        assert (c.GetCoverageByAmplicon(100, 100)[0] == -1).all() and int(c.GetCounts(100, 100).sum()) > 0
        refused(_abi.E_STATE, lambda: c.SetAmpliconBiasFilter(S.THRESHOLD))
    with caller(ref) as c:
        c.SetAmpliconBiasFilter(None)
        refused(_abi.E_STATE, lambda: c.GetCoverageByAmplicon(100))
        c.AddAlleleCounts(reads, amplicon_ids=ids)     # ids on a handle without the filter: the plain add
        rows = c.Call()
    assert rows.tobytes() == run("plain", ref, reads, ids, None).tobytes()
