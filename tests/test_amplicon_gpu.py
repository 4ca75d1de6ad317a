"""The amplicon-bias filter on the device (amplicon_kernels.hip.h): per-amplicon counts from the read store against the plain-Python
statement (tests/amplicon_ref.py), the filter bit of a flush against its decision, through every route a batch and a flush can take, the
six-slot limit, the refusals, and that a handle without the filter is untouched; then the same against seeded reads over a store's whole
life and seeded planted scenarios.  Scenarios and generators: tests/amplicon_cases.py."""
import functools

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import amplicon_cases as S
from tests import amplicon_ref as R
from tests.test_read_store import STORE_MODES, env, torch_cuda  # noqa: F401

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


def expected_bits(rows, ref, coverage, support, threshold=None):
    threshold = S.THRESHOLD if threshold is None else threshold
    want = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        if ((int(r["info"]) >> 4) & 7) != _abi.CAT_SNV or r["allele_support"] <= 0:
            continue
        p, alt = int(r["position"]), BASE_OF_TYPE[(int(r["info"]) >> 10) & 7]
        want[i] = R.bias_detected(support.get(p, {}).get(alt, {}), coverage.get(p, {}), threshold) is True
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


# ---- seeded fuzz: the generators of tests/amplicon_cases.py, whose promises tests/test_amplicon_cpu.py asserts without a device ----

FAR = (67000, S.FUZZ_REF_LENGTH)     # where the reads with a long skip land, and the reads that end on the reference's last base


@functools.lru_cache(maxsize=None)
def fuzz_reference():
    return S.reference(S.FUZZ_REF_LENGTH, seed=12)


def counts_of(reads, ids):
    """(coverage, support, untagged support) of the Python statement"""
    return R.amplicon_counts(reads, S.names_of(ids)) + (R.amplicon_counts(reads, [0 if i < 0 else None for i in ids])[1],)


@functools.lru_cache(maxsize=None)
def lifecycle(seed):
    """S.lifecycle_case(seed) and what the statement expects at its four stages: everything; the same (asked above the floor); with the batch
    that straddles the floor (below the floor that batch alone: the earlier reads' positions there are counted and gone); the fresh batch"""
    case = S.lifecycle_case(seed)
    first = counts_of(case["reads"], case["ids"])
    both = counts_of(case["reads"] + case["ahead"][0], case["ids"] + case["ahead"][1])
    ahead = counts_of(*case["ahead"])
    floor = case["floor"]
    merged = tuple({**{p: v for p, v in b.items() if p < floor}, **{p: v for p, v in a.items() if p >= floor}} for a, b in zip(both, ahead))
    return case, [first, first, merged, counts_of(*case["fresh"])]


def check_identity(c, lo, hi):
    """What holds whatever the bases are: support summed over the amplicons = the allele counts the caller itself uses (every read tagged),
    coverage = the support of the four bases added up"""
    ids, cov, sup = c.GetCoverageByAmplicon(lo, hi - lo + 1)
    folded = c.GetCounts(lo, hi - lo + 1).sum(axis=(2, 3))
    assert (sup.sum(axis=2) == folded[:, [BASE_OF_TYPE.index(b) for b in "ACGT"]]).all()
    assert (cov == sup.sum(axis=1)).all() and ((ids == -1) == (cov == 0)).all()
    return int(cov.sum())


def run_life(case, check, environment, in_order, device=False):
    """12 batches (more than the store has segments) -> check; Call(p) -> check what is held; a batch across the floor -> check;
    Call(), a batch with other ids over the same positions (retired and reset segments are used again) -> check"""
    reads, ids = case["reads"], case["ids"]
    if in_order:
        order = sorted(range(len(reads)), key=lambda k: reads[k]["pos"])
        reads, ids = [reads[k] for k in order], [ids[k] for k in order]
    floor = case["floor"]
    with env(PISCES_HIP_READ_PATH=None, **environment):
        with caller(fuzz_reference(), S.THRESHOLD) as c:
            add = (lambda r, i: c.AddDeviceReads(r, amplicon_ids=i)) if device else (lambda r, i: c.AddAlleleCounts(r, amplicon_ids=i))
            step = -(-len(reads) // 12)
            for k in range(0, len(reads), step):
                add(reads[k:k + step], ids[k:k + step])
            assert c.Stats()["reads"] == len(reads) and len(range(0, len(reads), step)) == 12
            for lo, hi in ((1, 130), (930, 1850), FAR):
                check(c, lo, hi, 0)
            rows = c.Call(case["call_at"])
            assert len(rows) and rows["position"].max() == floor - 1 and case["call_at"] % 1000 != 0
            assert (c.GetCoverageByAmplicon(930, floor - 930)[0] == -1).all()      # the flushed block holds nothing
            for lo, hi in ((floor, 1850), FAR):
                check(c, lo, hi, 1)
            add(*case["ahead"])
            assert case["ahead"][0][0]["pos"] < floor < case["ahead"][0][-1]["pos"]
            for lo, hi in ((floor - 60, 1850), FAR):
                check(c, lo, hi, 2)
            c.Call()
            assert (c.GetCoverageByAmplicon(930, 900)[0] == -1).all()
            add(*case["fresh"])
            for lo, hi in ((930, 1850), (FAR[0], FAR[0] + 100)):
                check(c, lo, hi, 3)
            c.Call()


@pytest.mark.parametrize("in_order", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("mode", list(STORE_MODES))
@pytest.mark.parametrize("seed", S.TAGGED_SEEDS)
def test_counts_of_seeded_reads_over_a_stores_life(torch_cuda, seed, mode, in_order):
    """Arbitrary CIGARs (= X H P N, clips, terminal deletions, reads without an aligned fragment, reads of a span above 0xFFFF), position 1
    and the reference's last base, 1..6 ids a position with 0 and 2^31 - 1 among them, against the Python statement: however the batches
    joined the store, in position order or not, before and after a floor, across it, and in segments that are used a second time."""
    case, expected = lifecycle(seed)
    run_life(case, lambda c, lo, hi, stage: check_counts(c, lo, hi, *expected[stage]), STORE_MODES[mode], in_order)


def test_counts_of_seeded_reads_handed_over_in_device_memory(torch_cuda):
    case, expected = lifecycle(S.TAGGED_SEEDS[0])
    run_life(case, lambda c, lo, hi, stage: check_counts(c, lo, hi, *expected[stage]), {}, False, device=True)


def test_counts_of_exotic_bases_add_up_to_the_callers_own(torch_cuda):
    """Bases that are no A C G T N, every read tagged: support summed over the amplicons = GetCounts folded, per A / C / G / T"""
    case = S.lifecycle_case(S.TAGGED_SEEDS[1], exotic=True, tag_all=True)
    seen = []
    run_life(case, lambda c, lo, hi, stage: seen.append(check_identity(c, lo, hi)), STORE_MODES["every batch appended to the open segment"], False)
    assert len(seen) == 9 and min(seen[:8]) > 0 and seen[8] == 0


# ---- the filter on planted scenarios ----

def is_snv(rows):
    return (((rows["info"] >> 4) & 7) == _abi.CAT_SNV) & (rows["allele_support"] > 0)


def snv_rows(rows, inside=None):
    """{(position, alternative base): (support, coverage, bit)} of the supported SNV rows (at the positions `inside` accepts)"""
    out = {}
    for r in rows[is_snv(rows)]:
        key = (int(r["position"]), BASE_OF_TYPE[(int(r["info"]) >> 10) & 7])
        assert key not in out
        if inside is None or inside(key[0]):
            out[key] = (int(r["allele_support"]), int(r["total_coverage"]), bool(int(r["filter_bits"]) & AB))
    return out


@functools.lru_cache(maxsize=None)
def planted_case(seed, threshold):
    sc = S.planted_scenario(seed, threshold)
    coverage, support = R.amplicon_counts(sc["reads"], S.names_of(sc["ids"]))
    total = R.amplicon_counts(sc["reads"], [0] * len(sc["reads"]))[1]
    return sc, coverage, support, total


def flagged_at_a_quarter(sc, coverage, support, total, threshold):
    """From the statement alone: does the scenario hold a flagged allele that every genotyper reports (a quarter of the depth or more)?"""
    for position, locus in sc["loci"].items():
        depth = sum(sum(by.values()) for by in total[position].values())
        for alt in locus["alts"]:
            if sum(total[position].get(alt, {}).values()) >= 0.25 * depth and R.bias_detected(support.get(position, {}).get(alt, {}), coverage[position], threshold):
                return True
    return False


def planted_rows(sc, route, filtered, cfg=None, environment=None, posteriors=False):
    """The rows of one planted scenario through one route, with the filter or without"""
    cfg = dict(cfg or {})
    reads, ids, threshold = sc["reads"], sc["ids"], sc["threshold"] if filtered else None
    if route == "streaming":
        cfg["block_size"] = 100
    with env(**(environment or {})):
        with caller(sc["ref"], threshold, **cfg) as c:
            if route == "intervals":
                c.SetIntervals(INTERVALS)
            if route == "owned":
                c.SetOwnedRange(*OWNED)
            if route == "streaming":     # SmallVariantCaller's schedule: add a stretch of reads, call up to their first position - 1
                rows = []
                for k in range(0, len(reads), 400):
                    c.AddAlleleCounts(reads[k:k + 400], amplicon_ids=ids[k:k + 400])
                    if reads[k]["pos"] > 1:
                        rows.append(c.Call(reads[k]["pos"] - 1))
                rows.append(c.Call())
                assert sum(len(r) > 0 for r in rows) >= 5      # reads were added behind several flushes
                return np.concatenate(rows)
            c.AddAlleleCounts(reads, amplicon_ids=ids)
            rows = c.Call()
            return (rows, c.Posteriors()) if posteriors else rows


INTERVALS = [(20, 75), (940, 1030), (1190, 1450), (1600, 1939)]     # start and end inside tiles; 76..939, a whole region behind 1030 and 1451..1599 left out
OWNED = (1, 1100)                                                    # cuts the second region


def in_intervals(p):
    return any(a <= p <= b for a, b in INTERVALS)


@pytest.mark.parametrize("seed,threshold", S.PLANTED_SEEDS)
def test_filter_on_planted_scenarios_equals_the_python_decision(torch_cuda, seed, threshold):
    """One batch, one flush: the rows with the filter are the rows without it but for the bit, the bit is the statement's decision at the
    scenario's threshold, and every planted allele of twice the minimum frequency has its row (a row without the bit is a decision)."""
    sc, coverage, support, total = planted_case(seed, threshold)
    rows, plain = planted_rows(sc, "one_shot", True), planted_rows(sc, "one_shot", False)
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, sc["ref"], coverage, support, threshold))
    snvs = snv_rows(rows)
    answers = {True: 0, False: 0, None: 0}
    for position, locus in sc["loci"].items():
        depth = sum(sum(by.values()) for by in total[position].values())
        for alt in locus["alts"]:
            carriers = sum(total[position].get(alt, {}).values())
            if carriers >= 2 * S.MIN_FREQUENCY * depth:
                assert (position, alt) in snvs, (position, alt, carriers, depth)
            if (position, alt) in snvs:
                want = R.bias_detected(support.get(position, {}).get(alt, {}), coverage[position], threshold)
                assert snvs[position, alt][2] is (want is True)
                answers[want] += 1
    assert min(answers.values()) >= 8, answers
    assert {1, len(sc["ref"]), 1001} <= {p for p, _ in snvs}
    assert any(len([a for a in locus["alts"] if (p, a) in snvs]) == 2 for p, locus in sc["loci"].items())   # two SNV rows on one locus


ROUTES = {
    "streaming schedule, blocks of 100": ("streaming", {}, {}),
    "intervals inside tiles": ("intervals", {}, {}),
    "owned range": ("owned", {}, {}),
    "tiles of 33 loci": ("one_shot", {}, dict(PISCES_HIP_TILE_LOCI="33")),
    "tiles of 59 loci": ("one_shot", {}, dict(PISCES_HIP_TILE_LOCI="59")),
    "compaction in two launches": ("one_shot", {}, dict(PISCES_HIP_COMPACT="two")),
    "compaction by look-back": ("one_shot", {}, dict(PISCES_HIP_COMPACT="lookback")),
    "genotypes by the host pass": ("one_shot", dict(ploidy=_abi.PLOIDY_DIPLOID), dict(PISCES_HIP_DEVICE_GENOTYPER=0)),
}


@pytest.mark.parametrize("name", list(ROUTES))
@pytest.mark.parametrize("seed,threshold", S.PLANTED_SEEDS)
def test_planted_scenarios_through_every_route(torch_cuda, seed, threshold, name):
    """Each route against itself without the filter and against the statement, and its SNV rows (support, coverage, bit) against the one
    flush of the same scenario: all of them where the route reports (inside the intervals, inside the owned range), and nothing else."""
    route, cfg, environment = ROUTES[name]
    sc, coverage, support, total = planted_case(seed, threshold)
    rows, plain = planted_rows(sc, route, True, cfg, environment), planted_rows(sc, route, False, cfg, environment)
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, sc["ref"], coverage, support, threshold))
    inside = {"intervals": in_intervals, "owned": lambda p: OWNED[0] <= p <= OWNED[1]}.get(route)
    one_shot = snv_rows(planted_rows(sc, "one_shot", True, cfg))
    got = snv_rows(rows)
    assert got.items() <= one_shot.items()
    assert snv_rows(rows, inside) == {k: v for k, v in one_shot.items() if inside is None or inside(k[0])}
    assert not all(bit for _, _, bit in got.values())
    assert any(bit for _, _, bit in got.values()) or (cfg and not flagged_at_a_quarter(sc, coverage, support, total, threshold))
    if route == "intervals":
        assert all(in_intervals(int(p)) for p in rows["position"])


@pytest.mark.parametrize("seed,threshold", S.PLANTED_SEEDS)
def test_planted_scenarios_under_the_other_genotypers_and_with_reference_rows(torch_cuda, seed, threshold):
    sc, coverage, support, total = planted_case(seed, threshold)
    # DiploidByAdaptiveGT: the genotyper runs right behind the pass; rows but for the bit, and the posteriors, as without the filter
    (rows, post), (plain, plain_post) = (planted_rows(sc, "one_shot", on, dict(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE), posteriors=True) for on in (True, False))
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, sc["ref"], coverage, support, threshold))
    assert len(post) == len(rows) and post.tobytes() == plain_post.tobytes() and (post["n"] > 0).any()
    assert ((rows["filter_bits"] & AB) != 0).any() or not flagged_at_a_quarter(sc, coverage, support, total, threshold)
    # haploid: (the scenario's alleles stay below the 70 % the genotyper asks of a locus' one allele: see the haploid scenario below)
    rows, plain = (planted_rows(sc, "one_shot", on, dict(ploidy=_abi.PLOIDY_HAPLOID)) for on in (True, False))
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, sc["ref"], coverage, support, threshold))
    # gVCF: reference rows at every position, covered or not; none of them ever carries the bit
    rows, plain = (planted_rows(sc, "one_shot", on, dict(emit_zero_coverage_refs=1)) for on in (True, False))
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, sc["ref"], coverage, support, threshold))
    reference_rows = ((rows["info"] >> 4) & 7) == _abi.CAT_REFERENCE
    assert reference_rows.sum() > 500 and not (rows["filter_bits"][reference_rows] & AB).any()
    assert (rows["filter_bits"][is_snv(rows)] & AB).any()


def test_haploid_genotyper_keeps_the_bit_on_the_allele_it_reports(torch_cuda):
    ref, reads, ids = S.haploid_scenario()
    coverage, support = R.amplicon_counts(reads, S.names_of(ids))
    rows, plain = (run("plain", ref, reads, ids, threshold, ploidy=_abi.PLOIDY_HAPLOID) for threshold in (S.THRESHOLD, None))
    assert_only_the_bit_differs(rows, plain, expected_bits(rows, ref, coverage, support))
    assert {p: bit for (p, _), (_, _, bit) in snv_rows(rows).items()} == S.HAPLOID_PLANTED


def test_twenty_runs_give_the_same_bytes(torch_cuda):
    """The slots of a locus are claimed in arrival order, which differs from run to run: neither the rows nor the sorted counts may"""
    sc = planted_case(*S.PLANTED_SEEDS[0])[0]
    n, seen = len(sc["ref"]), set()
    for _ in range(20):
        with caller(sc["ref"], sc["threshold"]) as c:
            c.AddAlleleCounts(sc["reads"], amplicon_ids=sc["ids"])
            ids, cov, sup = c.GetCoverageByAmplicon(1, n)
            seen.add((ids.tobytes(), cov.tobytes(), sup.tobytes(), c.Call().tobytes()))
    assert len(seen) == 1


def test_a_seventh_amplicon_in_two_tiles_names_the_lowest_position_that_matters(torch_cuda):
    """Seventh ids at 70 (tile 65..128, no SNV) and at 200 (tile 193..256, an SNV at 205), neither a tile's first position: the counts
    over the range name 70; the flush, which counts in tiles that hold a supported SNV row only, names 200; the blocks stay held."""
    ref = S.reference()
    reads = [S._read(ref, 70, [("M", 5)]) for _ in range(70)] + [S._read(ref, 200, [("M", 10)], edits={205: S.OTHER[chr(ref[204])]}) for _ in range(70)]
    ids = [10 + i % 7 for i in range(70)] + [1000 + i % 7 for i in range(70)]
    with caller(ref, S.THRESHOLD) as c:
        c.AddAlleleCounts(reads, amplicon_ids=ids)
        for failing, position in ((lambda: c.GetCoverageByAmplicon(1, 300), 70), (c.Call, 200), (lambda: c.GetCoverageByAmplicon(60, 200), 70)):
            with pytest.raises(engine.PiscesHipError) as e:
                failing()
            assert e.value.code == _abi.E_INVALID_ARG and "more than 6 amplicons" in e.value.message and f"position {position})" in e.value.message
            assert int(c.GetCounts(70, 1).sum()) == 70 and int(c.GetCounts(200, 1).sum()) == 70     # the blocks stay held
