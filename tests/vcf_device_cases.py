"""Seeded rows for the device VCF formatter (pisces_hip_format_vcf_device), shared by tests/test_vcf_device_cpu.py (the generator keeps
its promises) and tests/test_vcf_device_gpu.py (device bytes == host bytes).  Nothing here calls the library: the rounding oracle is
Python's decimal on the exact value of the float32 quotient."""
import decimal
import math

import numpy as np

from pisces_amd import _abi

D = decimal.Decimal
N_GENOTYPES = 13          # PISCES_GT_* 0..12
N_CATEGORIES = 5          # PISCES_CAT_* 0..4
FILTER_BITS = 14          # filter_bits 0..13 (14..15 carry PhaseSetIndex); 1, 7, 11 and 13 have no name: the host formatter ignores them
ALL_FILTERS = (1 << FILTER_BITS) - 1
CAT_SNV, CAT_REF = 0, 4
GT_ALT12, GT_HET, GT_OTHERS = 0, 2, 12

# strand_bias_score edge values (rows that carry them have support > 0, so the SB column is computed from them)
SB_EDGES = ([float("nan"), 0.0, -0.5, -1e-300, 1.5, 1e300] + [10.0 ** -k for k in range(1, 11)] +
            [math.nextafter(1.0, 0.0), math.nextafter(1.0, 2.0), 1.0,
             10.0 ** (-0.00004 / 10.0),      # 10 log10 = -0.00004: "0.0000" from below, without the sign
             10.0 ** (-0.00005 / 10.0), 10.0 ** (-0.00006 / 10.0), 1e-11, 1e-12, 5e-324])
GP_VALUES = [0.0, 3000.0, float("nan"), 2.675, 0.005, 0.004999, 12.345, 2999.995, float("inf"), -0.001, 1e7, 16777216.0, 3.4e38]


def two_step(value, sig, decimals):
    """Single/Double.ToString("0.000") of .NET Core 2.0 on the exact binary `value`: `sig` significant digits (7 / 15), then half-up."""
    if value == 0:
        first = D(0)
    else:
        v = D(value)   # exact
        first = v.quantize(D(1).scaleb(v.adjusted() - (sig - 1)), rounding=decimal.ROUND_HALF_EVEN)
    return first.quantize(D(1).scaleb(-decimals), rounding=decimal.ROUND_HALF_UP)


def one_step(value, decimals):
    return D(value).quantize(D(1).scaleb(-decimals), rounding=decimal.ROUND_HALF_UP)


def frequency(support, coverage):
    """CalledAllele.Frequency as the formatter computes it: a float32 quotient (IEEE division, numpy's), at most 1"""
    if coverage == 0:
        return 0.0
    f = np.float32(support) / np.float32(coverage)
    return float(min(f, np.float32(1.0)))


def rounding_differs(support, coverage, decimals):
    f = frequency(support, coverage)
    return two_step(f, 7, decimals) != one_step(f, decimals)


def _row(rng):
    r = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)
    g = np.zeros(1, dtype=_abi.POSTERIORS_DTYPE)
    return r, g


def _info(gt, cat, ref, alt):
    return gt | (cat << 4) | (ref << 7) | (alt << 10)


def _fill_common(rng, r, g):
    r["position"] = int(rng.integers(1, 250_000_000))
    r["variant_qscore"] = int(rng.integers(0, 101))
    r["genotype_qscore"] = int(rng.integers(0, 101))
    r["num_no_calls"] = 0 if rng.integers(0, 3) else int(rng.integers(0, 500))
    r["noise_level"] = -32768 if rng.integers(0, 25) == 0 else int(rng.integers(0, 60))
    r["strand_bias_score"] = SB_EDGES[int(rng.integers(0, len(SB_EDGES)))] if rng.integers(0, 4) == 0 else (
        float(rng.random()) if rng.integers(0, 2) else 10.0 ** (-12.0 * float(rng.random())))
    k = int(rng.integers(0, 4))
    g["n"] = (0, 3, 6, 3)[k]
    for j in range(6):
        g["gp"][0][j] = GP_VALUES[int(rng.integers(0, len(GP_VALUES)))] if rng.integers(0, 3) == 0 else float(rng.integers(0, 3_000_000)) / 1000.0


def generate(n=5000, seed=20261019, need_differing=200, decimals=(3, 5)):
    """(rows, posteriors, stats): at least `n` seeded rows, drawn until for every entry of `decimals` at least `need_differing` of them
    are plain 0/1 SNV rows whose VF differs between two-step and one-step rounding.  No drawn row is discarded (stats["discarded"] is
    what the 1 % cap is held against).  The first rows are the systematic ones: every genotype, category and filter bit, the named edge
    cases; then a seeded mix in which a share of the rows sits on a half unit of the last VF decimal (support / coverage =
    (2j + 1) / (2 * 10^d), not a binary fraction: the float32 quotient lies just below or just above the half, and below it the first
    rounding lifts the digit string onto the half)."""
    rng = np.random.default_rng(seed)
    rows, gps = [], []

    def add(r, g):
        rows.append(r)
        gps.append(g)

    # every genotype x every category
    for gt in range(N_GENOTYPES):
        for cat in range(N_CATEGORIES):
            r, g = _row(rng)
            _fill_common(rng, r, g)
            cov = int(rng.integers(1, 2001))
            sup = int(rng.integers(0, cov + 1))
            r["total_coverage"], r["allele_support"], r["reference_support"] = cov, sup, int(rng.integers(0, cov - sup + 1))
            r["info"] = _info(gt, cat, int(rng.integers(0, 6)), int(rng.integers(0, 6)))
            r["filter_bits"] = int(rng.integers(0, 3)) << 14
            add(r, g)
    # every filter bit alone, all together, with each phase
    for bits in [1 << b for b in range(FILTER_BITS)] + [ALL_FILTERS, 0]:
        for phase in range(3):
            r, g = _row(rng)
            _fill_common(rng, r, g)
            r["total_coverage"], r["allele_support"], r["reference_support"] = 1000, 250, 700
            r["info"] = _info(GT_HET, CAT_SNV, 0, 3)
            r["filter_bits"] = bits | (phase << 14)
            add(r, g)
    # the SB edges on rows with support
    for sb in SB_EDGES:
        r, g = _row(rng)
        _fill_common(rng, r, g)
        r["total_coverage"], r["allele_support"], r["reference_support"] = 500, 100, 400
        r["strand_bias_score"] = sb
        r["info"] = _info(GT_HET, CAT_SNV, 1, 2)
        add(r, g)
    # coverage 0, support > coverage, noise_level -32768, 1/2 and forced rows of every phase, GP of every shape and value
    for (cov, sup, rs) in [(0, 0, 0), (10, 15, 2), (10, 15, 20), (7, 0, 7), (1, 1, 0), (2000, 1999, 1), (100000, 5000, 95000), (3, 1, 2), (16, 1, 15)]:
        for (gt, cat) in [(GT_HET, CAT_SNV), (4, CAT_REF), (GT_ALT12, CAT_SNV), (GT_OTHERS, CAT_SNV), (1, CAT_SNV)]:
            for phase in range(3):
                r, g = _row(rng)
                _fill_common(rng, r, g)
                r["total_coverage"], r["allele_support"], r["reference_support"] = cov, sup, rs
                r["noise_level"] = -32768 if phase == 0 else int(r["noise_level"][0])
                r["info"] = _info(gt, cat, 2, 3)
                r["filter_bits"] = (phase << 14) | ((1 << 10) if (cov + phase) % 2 else 0)
                add(r, g)
    for n_gp in (0, 3, 6):
        for v in GP_VALUES:
            r, g = _row(rng)
            _fill_common(rng, r, g)
            r["total_coverage"], r["allele_support"], r["reference_support"] = 60, 30, 30
            r["info"] = _info(GT_HET, CAT_SNV, 0, 1)
            g["n"] = n_gp
            g["gp"][0][:] = v
            add(r, g)
    systematic = len(rows)
    differing = {d: 0 for d in decimals}
    drawn = systematic
    while len(rows) < n or any(differing[d] < need_differing for d in decimals):
        assert drawn < 4 * n + 4 * systematic, "the generator does not reach its promises"
        r, g = _row(rng)
        _fill_common(rng, r, g)
        kind = int(rng.integers(0, 10))
        if kind < 2 * len(decimals):   # on a half unit of decimal d
            d = decimals[kind % len(decimals)]
            cov = 2 * 10 ** d
            sup = 2 * int(rng.integers(0, 10 ** d)) + 1
            r["total_coverage"], r["allele_support"], r["reference_support"] = cov, sup, cov - sup
            r["info"] = _info(GT_HET, CAT_SNV, int(rng.integers(0, 4)), int(rng.integers(0, 4)))
            if rounding_differs(sup, cov, d):
                differing[d] += 1
        else:
            cov = int(rng.integers(0, 2001)) if rng.integers(0, 4) else int(rng.integers(0, 200_000))
            sup = int(rng.integers(0, cov + 1))
            if rng.integers(0, 40) == 0:
                sup = cov + int(rng.integers(1, 10))
            rs = int(rng.integers(0, cov - sup + 1)) if cov >= sup else int(rng.integers(0, 5))
            r["total_coverage"], r["allele_support"], r["reference_support"] = cov, sup, rs
            gt = int(rng.integers(0, N_GENOTYPES))
            cat = CAT_REF if rng.integers(0, 3) == 0 else int(rng.integers(0, 4))
            r["info"] = _info(gt, cat, int(rng.integers(0, 6)), int(rng.integers(0, 6)))
            bits = int(rng.integers(0, 1 << FILTER_BITS)) if rng.integers(0, 3) == 0 else 0
            r["filter_bits"] = bits | (int(rng.integers(0, 3)) << 14)
        add(r, g)
        drawn += 1
    stats = {"drawn": drawn, "discarded": drawn - len(rows), "systematic": systematic, "differing": differing}
    return np.concatenate(rows), np.concatenate(gps), stats


_CACHE = {}


def cases():
    """generate() with its defaults, made once a process and handed out read-only"""
    if "v" not in _CACHE:
        rows, gps, stats = generate()
        rows.setflags(write=False)
        gps.setflags(write=False)
        _CACHE["v"] = (rows, gps, stats)
    return _CACHE["v"]


def allele_cases(lengths=(1, 63, 64, 300), point_rows_between=5, seed=7):
    """(rows, alleles): insertion / deletion / MNV rows whose allele strings have the given lengths, next to point rows (alleles as
    engine.format_vcf takes them; a (ref, alt) of two single bases is a row without a candidate)."""
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    rows, alleles = [], []
    pos = 1000
    for ln in lengths:
        for (cat, ref_n, alt_n) in [(1, 1, ln + 1), (2, ln + 1, 1), (3, ln, ln)]:   # insertion, deletion, MNV
            if cat == 3 and ln == 1:
                continue
            for gt, phase in [(GT_HET, 0), (GT_ALT12, 1), (GT_ALT12, 2)]:
                for _ in range(point_rows_between):
                    r = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)
                    pos += 1
                    r["position"], r["total_coverage"], r["allele_support"], r["reference_support"] = pos, 400, 100, 300
                    r["strand_bias_score"], r["variant_qscore"], r["genotype_qscore"] = 0.5, 100, 50
                    a, b = int(rng.integers(0, 4)), int(rng.integers(0, 4))
                    r["info"] = _info(GT_HET, CAT_SNV, a, b)
                    rows.append(r)
                    alleles.append(("AGCT"[a], "AGCT"[b]))
                r = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)
                pos += 1
                r["position"], r["total_coverage"], r["allele_support"], r["reference_support"] = pos, 400, 120, 200
                r["strand_bias_score"], r["variant_qscore"], r["genotype_qscore"] = 0.25, 100, 50
                r["info"] = _info(gt, cat, 0, 4)
                r["filter_bits"] = phase << 14
                rows.append(r)
                alleles.append(("".join(letters[int(x)] for x in rng.integers(0, 4, ref_n)), "".join(letters[int(x)] for x in rng.integers(0, 4, alt_n))))
    return np.concatenate(rows), alleles
