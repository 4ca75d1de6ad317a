"""The amplicon-bias filter (-abfilter, FILTER AB) in plain Python: the yardstick of tests/test_amplicon_cpu.py.

A statement of
  src/lib/Pisces.Processing/RegionState/RegionStateManager.cs:143-193     AddAlleleCounts: which bases reach AddAmpliconCount
  src/lib/Pisces.Processing/RegionState/RegionState.cs:269-307            AddAmpliconCount: six name slots a position, a null name counts nothing
  src/lib/Pisces.Domain/Logic/CandidateVariantFinder.cs:205-232           an SNV's SupportByAmplicon: {name: 1} per supporting read
  src/lib/Pisces.Calculators/AmpliconBiasCalculator.cs:45-134             CalculateAmpliconBias
with names as Python objects (None = no XN tag) and counts in dicts.  It shares no code with the library: Poisson.Cdf is the oracle's
orc_poisson_cdf, which tests/test_oracle_golden.py pins to the reference's tables; tests/test_amplicon_cpu.py first holds the decision
to the reference's own unit tests (tests/golden/amplicon_bias_cases.json)."""
import numpy as np

from tests import orc

MAX_OVERLAPPING_AMPLICONS = 6      # Constants.MaxNumOverlappingAmplicons
MIN_NUM_OBSERVATIONS = 5           # AmpliconBiasCalculator.Constants
FREE_PASS_OBSERVATION_FREQ = 0.1


def poisson_cdf(num_occurrences, expected):
    return float(orc.lib.orc_poisson_cdf(float(num_occurrences), float(expected)))


class TooManyAmplicons(Exception):
    """The seventh name of a position: RegionState.AddAmpliconCount indexes slot -1 and the reference throws IndexOutOfRangeException."""
    def __init__(self, position):
        super().__init__(f"more than {MAX_OVERLAPPING_AMPLICONS} amplicons at position {position}")
        self.position = position


def reference_positions(read):
    """(index into the read's bases, 1-based reference position) of every base that Read.PositionMap maps: M / = / X consume both,
    I and S the read alone, D and N the reference alone, H and P nothing."""
    pos, i = int(read["pos"]), 0
    for op, length in read["cigar"]:
        if op in "M=X":
            for k in range(length):
                yield i + k, pos + k
            i += length
            pos += length
        elif op in "IS":
            i += length
        elif op in "DN":
            pos += length


def amplicon_counts(reads, names, min_base_call_quality=20):
    """reads: the dicts _abi.ReadBatch takes; names[i]: read i's amplicon (any hashable), None without a tag.
    -> (coverage, support): coverage[position] = {name: count of the A/C/G/T bases at or above the minimum quality that tagged reads bring},
    support[position][base] = the same split by the base (with MNV calling off, what an SNV to that base has as SupportByAmplicon).
    Positions and names nobody counted at are absent; deleted positions, N bases and low-quality bases count nowhere."""
    coverage, support = {}, {}
    for read, name in zip(reads, names):
        if name is None:
            continue
        seq = read["seq"] if isinstance(read["seq"], str) else bytes(read["seq"]).decode()
        quals = bytes(read["quals"])
        for i, position in reference_positions(read):
            base = seq[i]
            if base not in "ACGT" or quals[i] < min_base_call_quality:
                continue
            slots = coverage.setdefault(position, {})
            if name not in slots and len(slots) == MAX_OVERLAPPING_AMPLICONS:
                raise TooManyAmplicons(position)
            slots[name] = slots.get(name, 0) + 1
            by_base = support.setdefault(position, {}).setdefault(base, {})
            by_base[name] = by_base.get(name, 0) + 1
    return coverage, support


def chances(support_by_amplicon, coverage_by_amplicon):
    """pChanceItsReal of every amplicon of the coverage list, in its order; None where CalculateAmpliconBias returns null."""
    if not support_by_amplicon:                      # no names, or a first name that is null
        return None
    if len(coverage_by_amplicon) < 2:
        return None
    rows, max_freq = [], 0.0
    for name, coverage in coverage_by_amplicon.items():
        support = float(support_by_amplicon.get(name, 0))     # AmpliconCounts.GetCountsForAmplicon: 0 for a name it does not hold
        coverage = float(coverage)
        freq = support / coverage if coverage > 0 else 0.0
        if freq >= max_freq:
            max_freq = freq
        rows.append((support, coverage, freq))
    out = []
    for support, coverage, freq in rows:
        expected = max_freq * coverage
        p = 1.0
        if expected < MIN_NUM_OBSERVATIONS:
            pass
        elif expected <= support or freq > FREE_PASS_OBSERVATION_FREQ:
            pass
        else:
            p = max(0.0, poisson_cdf(support, expected))
        out.append(p)
    return out


def bias_detected(support_by_amplicon, coverage_by_amplicon, threshold):
    """BiasResultsAcrossAmplicons.BiasDetected (True / False), or None for a null result.  threshold is the float? of the option."""
    p = chances(support_by_amplicon, coverage_by_amplicon)
    if p is None:
        return None
    allowable = float(np.float32(threshold))
    return any(x < allowable for x in p)


def margin_to_threshold(support_by_amplicon, coverage_by_amplicon, threshold):
    """The smallest |p_i - threshold| / threshold over the amplicons (inf for a null result or a zero threshold): how far a case is from
    changing its answer under a rounding difference in Poisson.Cdf."""
    p = chances(support_by_amplicon, coverage_by_amplicon)
    allowable = float(np.float32(threshold))
    if p is None or allowable == 0.0:
        return float("inf")
    return min(abs(x - allowable) / allowable for x in p)
