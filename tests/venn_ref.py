"""VennVcf's consensus of two probe pools stated in plain Python over dicts, for the tests of the pisces_hip_venn_* entries.  It follows the
reference's files line by line (src/exe/VennVcf/VennVcf.cs, ConsensusBuilder.cs; CalledAllele.cs, BaseAllele.cs) and shares no code with the
library: the objects are mutable as the reference's are (DoDefensiveGenotyping and PushThroughRamificationsOfGTChange write into their inputs),
where the library carries that state explicitly.  The two things it does not restate are VariantQualityCalculator.AssignPoissonQScore and
StrandBiasCalculator.CalculateStrandBiasResults: the oracle's orc_poisson_qscore and orc_strand_bias.

A row is a dict: position, ref, alt (strings; "." is a reference call's alt), type, genotype (a Genotype name), total_coverage, allele_support,
reference_support, variant_qscore, genotype_qscore, noise_level, filters (bit i = FilterType i), sb (StrandBiasResults.BiasScore, whose
10 * log10 is the GATK score), and what the library's rows carry beside: num_no_calls, coverage_by_dir, support_by_dir, bias_bits.
"""
import copy
import math

import numpy as np

from tests import orc

# index = PISCES_GT_*
GENOTYPES = ("HeterozygousAlt1Alt2", "Alt12LikeNoCall", "HeterozygousAltRef", "HomozygousAlt", "HomozygousRef", "RefLikeNoCall", "AltLikeNoCall",
             "RefAndNoCall", "AltAndNoCall", "HemizygousRef", "HemizygousAlt", "HemizygousNoCall", "Others")
TYPES = ("Snv", "Insertion", "Deletion", "Mnv", "Reference")   # index = PISCES_CAT_*
CASES = ("AgreedOnReference", "AgreedOnAlternate", "OneReferenceOneAlternate", "CanNotCombine")
INT_MIN = -2147483648
FILTER_POOL_BIAS = 1
SB_EXTENDED = 1
TAKE_MIN = 1


def default_options(**overrides):
    """VennVcfOptions as far as the consensus reads them; the thresholds are Singles in the reference"""
    o = {"min_frequency": 0.01, "min_frequency_filter": 0.01, "pool_bias_threshold": 0.5, "min_coverage": 10, "max_variant_qscore": 100,
         "combine_qscore_method": 0}
    o.update(overrides)
    return o


def _single(x):
    return float(np.float32(x))


def set_type(ref, alt):   # BaseAllele.CalculateType (BaseAllele.cs:50-76)
    if ref and alt:
        if ref.lower() == alt.lower():
            return "Reference"
        if alt == ".":
            return "Reference"
        if len(ref) == len(alt):
            return "Snv" if len(alt) == 1 else "Mnv"
        if len(ref) == 1:
            return "Insertion"
        if len(alt) == 1:
            return "Deletion"
    return "Unsupported"


def math_max(x, y):   # Math.Max: a NaN on either side gives a NaN (an input's SB column may read "NaN")
    return float("nan") if x != x or y != y else max(x, y)


def has_a_ref_allele(v):   # CalledAllele.cs:80-89
    return v["genotype"] in ("RefAndNoCall", "HomozygousRef", "HemizygousRef", "HeterozygousAltRef")


def has_an_alt_allele(v):   # CalledAllele.cs:91-100
    return v["genotype"] in ("AltAndNoCall", "HomozygousAlt", "HeterozygousAlt1Alt2", "HeterozygousAltRef")


def q_to_p(q):
    if q == INT_MIN:
        return float("inf")
    return math.pow(10.0, -1 * float(q) / 10.0)


def assign_poisson_qscore(call_count, coverage, noise_level, max_qscore):   # VariantQualityCalculator.cs:54-65
    if call_count <= 0 or coverage <= 0:
        return 0
    if noise_level == INT_MIN:   # lambda = +infinity: the CDF is 0, p = 1, Q = 0
        return 0
    return int(orc.lib.orc_poisson_qscore(int(call_count), int(coverage), int(noise_level), int(max_qscore)))


# ---- VennVcf.cs ---------------------------------------------------------------------------------------------------------------------
def select_pairs(pool_a, pool_b):   # :420-487
    results = []
    if len(pool_a) == 1 and pool_a[0]["alt"] == ".":
        for b in pool_b:
            results.append((pool_a[0], b))
        if len(pool_b) == 0:
            results.append((pool_a[0], None))
    elif len(pool_b) == 1 and pool_b[0]["alt"] == ".":
        for a in pool_a:
            results.append((a, pool_b[0]))
        if len(pool_a) == 0:
            results.append((None, pool_b[0]))
    else:
        matched = []
        for a in pool_a:
            found = False
            for j, b in enumerate(pool_b):
                if a["ref"] == b["ref"] and a["alt"] == b["alt"]:
                    results.append((a, b))
                    matched.append(j)
                    found = True
                    break
            if not found:
                results.append((a, None))
        for j, b in enumerate(pool_b):
            if j not in matched:
                results.append((None, b))
    return results


def comparison_case(a, b):   # :489-537
    if a is None or b is None:
        return "CanNotCombine"
    if a["position"] != b["position"]:
        raise ValueError("Check input variants to var compare algs.")
    ref_a, ref_b = a["type"] == "Reference", b["type"] == "Reference"
    if ref_a and ref_b:
        return "AgreedOnReference"
    if ref_a != ref_b:
        return "OneReferenceOneAlternate"
    if a["ref"] == b["ref"] and a["alt"] == b["alt"]:
        return "AgreedOnAlternate"
    raise ValueError("Check input variants to var compare algs.")


# ---- ConsensusBuilder.cs --------------------------------------------------------------------------------------------------------------
def do_defensive_genotyping(v):   # :82-95
    if v["genotype"] in ("AltAndNoCall", "HemizygousAlt"):
        v["genotype"] = "HomozygousAlt"
    if v["genotype"] in ("RefAndNoCall", "HemizygousRef"):
        v["genotype"] = "HomozygousRef"
    if v["genotype"] == "HemizygousNoCall":
        v["genotype"] = "RefLikeNoCall"
    return v["genotype"]


def combine_noise_levels_by_taking_avg_p(nl1, nl2):   # :458-467
    if nl1 == nl2:
        return nl1
    p = (q_to_p(nl1) + q_to_p(nl2)) / 2.0
    if p == float("inf"):
        return INT_MIN
    return int(round(-10 * math.log10(p)))   # Math.Round, ties to even, as Python's


def get_genotype(a, b, case, total_depth, vf, vf_a, vf_b, o, taken):   # :304-398
    ref_present = (a is not None and has_a_ref_allele(a)) or (b is not None and has_a_ref_allele(b))
    alt_present = (a is not None and has_an_alt_allele(a)) or (b is not None and has_an_alt_allele(b))
    if not alt_present and ref_present:
        gt = "HomozygousRef"
    elif alt_present and ref_present:
        gt = "HeterozygousAltRef"
    elif alt_present and not ref_present:
        gt = "HomozygousAlt"
    else:
        gt = "RefLikeNoCall"
    if gt == "RefLikeNoCall":
        taken.add("gt:nothing-present")
        return gt
    mf, mff = _single(o["min_frequency"]), _single(o["min_frequency_filter"])
    if case != "AgreedOnReference":
        if vf < mf:
            if vf_a < mff and vf_b < mff:
                taken.add("gt:below-min-frequency-both-pools-low")
                gt = "HomozygousRef"
            else:
                taken.add("gt:below-min-frequency-one-pool-high")
                gt = "AltLikeNoCall"
        elif vf < mff:
            taken.add("gt:below-filter-frequency")
            gt = "AltLikeNoCall"
        else:
            taken.add("gt:kept")
    elif total_depth < o["min_coverage"]:
        taken.add("gt:low-depth")
        gt = "RefLikeNoCall"
    else:
        taken.add("gt:reference-kept")
    return gt


def combine_variants(a, b, case, o, taken=None):
    """CombineVariants (:36-80) with RecalculateScoring (:158-245).  a and b are changed as the reference changes them."""
    taken = taken if taken is not None else set()
    taken.add("case:" + case)
    for v in (a, b):
        if v is not None:
            before = v["genotype"]
            if do_defensive_genotyping(v) != before:
                taken.add("defensive:" + before)
    # CombineReferenceAlleles / CombineVariantAlleles (:99-156)
    if case in ("AgreedOnReference", "AgreedOnAlternate"):
        src = a
    elif case == "OneReferenceOneAlternate":
        src = b if a["type"] == "Reference" else a
    else:
        src = a if b is None else b
    c = {"position": (b if b is not None else a)["position"], "ref": src["ref"], "alt": "." if case == "AgreedOnReference" else src["alt"]}
    filters = 0
    for v in (a, b):   # CombineFilters / MergeFilters (VcfFormatter.cs:423-431)
        if v is not None:
            filters |= v["filters"]
    # RecalculateScoring
    ref_count_a = a["reference_support"] if a is not None else 0
    alt_count_a = (0 if a["type"] == "Reference" else a["allele_support"]) if a is not None else 0
    depth_a = a["total_coverage"] if a is not None else 0
    ref_count_b = b["reference_support"] if b is not None else 0
    alt_count_b = (0 if b["type"] == "Reference" else b["allele_support"]) if b is not None else 0
    depth_b = b["total_coverage"] if b is not None else 0
    total_depth, reference_depth, alt_depth = depth_a + depth_b, ref_count_a + ref_count_b, alt_count_a + alt_count_b
    vf = 0.0 if alt_depth == 0 or total_depth == 0 else alt_depth / total_depth
    vf_a = 0.0 if alt_count_a == 0 or depth_a == 0 else alt_count_a / depth_a
    vf_b = 0.0 if alt_count_b == 0 or depth_b == 0 else alt_count_b / depth_b
    c["total_coverage"], c["allele_support"], c["reference_support"] = total_depth, alt_depth, reference_depth
    gt = get_genotype(a, b, case, total_depth, vf, vf_a, vf_b, o, taken)
    take_min = o["combine_qscore_method"] == TAKE_MIN
    taken.add("method:take-min" if take_min else "method:pool")
    # GetCombinedNLValue (:290-302) / GetCombinedSBValue (:277-289)
    if a is None:
        nl, sb = b["noise_level"], b["sb"]
    elif b is None:
        nl, sb = a["noise_level"], a["sb"]
    else:
        if a["noise_level"] != b["noise_level"]:
            taken.add("noise-levels-differ")
        nl = min(a["noise_level"], b["noise_level"]) if take_min else combine_noise_levels_by_taking_avg_p(a["noise_level"], b["noise_level"])
        sb = math_max(a["sb"], b["sb"])
    c["noise_level"], c["sb"] = nl, sb
    # PushThroughRamificationsOfGTChange (:247-275)
    changed = gt in ("HomozygousRef", "RefLikeNoCall") and case == "OneReferenceOneAlternate"
    if changed:
        taken.add("alt-changed-to-ref")
        c["alt"] = "."
        c["ref"] = c["ref"][:1]
        if a is not None:
            a["variant_qscore"] = assign_poisson_qscore(ref_count_a, depth_a, nl, o["max_variant_qscore"])
        if b is not None:
            b["variant_qscore"] = assign_poisson_qscore(ref_count_b, depth_b, nl, o["max_variant_qscore"])
        c["allele_support"] = c["reference_support"]
    c["genotype"] = gt
    # GetProbePoolBiasScore (:401-455)
    pb_score, pb_gatk = 0.0, -100.0
    if changed or case == "AgreedOnReference":
        pass
    elif case in ("OneReferenceOneAlternate", "CanNotCombine"):
        filters |= 1 << FILTER_POOL_BIAS
        pb_gatk, pb_score = 0.0, 1.0
    else:
        r = orc.strand_bias([depth_a, depth_b, 0], [alt_count_a, alt_count_b, 0], q_noise=0 if nl == INT_MIN else nl, min_vf=_single(o["min_frequency"]),
                            acceptance=_single(o["pool_bias_threshold"]), model=SB_EXTENDED)
        pb_gatk = max(-100.0, min(0.0, r.gatk_bias_score))
        pb_score = min(1.0, r.bias_score)
        if not r.bias_acceptable:
            taken.add("pool-bias:biased")
            filters |= 1 << FILTER_POOL_BIAS
        else:
            taken.add("pool-bias:acceptable")
    c["filters"], c["pb_score"], c["pb_gatk"] = filters, pb_score, pb_gatk
    # the q-score (:215-237)
    if take_min:
        if b is None:
            vq = a["variant_qscore"]
        elif a is None:
            vq = b["variant_qscore"]
        else:
            vq = min(a["variant_qscore"], b["variant_qscore"])
    elif case == "AgreedOnReference" or (case == "OneReferenceOneAlternate" and changed) or (case == "CanNotCombine" and alt_depth == 0):
        if case == "CanNotCombine":
            taken.add("cannot-combine-reference-model")
        vq = assign_poisson_qscore(reference_depth, total_depth, nl, o["max_variant_qscore"])
    else:
        vq = assign_poisson_qscore(alt_depth, total_depth, nl, o["max_variant_qscore"])
    c["variant_qscore"] = c["genotype_qscore"] = vq
    c["type"] = set_type(c["ref"], c["alt"])
    if c["type"] == "Reference":
        c["allele_support"] = c["reference_support"]
    # the library's own fields
    members = [v for v in (a, b) if v is not None]
    c["num_no_calls"] = sum(v.get("num_no_calls", 0) for v in members)
    c["coverage_by_dir"] = [sum(v.get("coverage_by_dir", [0, 0, 0])[d] for v in members) for d in range(3)]
    c["support_by_dir"] = [sum(v.get("support_by_dir", [0, 0, 0])[d] for v in members) for d in range(3)]
    c["bias_bits"] = 0
    for v in members:
        c["bias_bits"] |= v.get("bias_bits", 0)
    c["case"], c["alt_changed_to_ref"] = case, changed
    return c


def venn_classes(case, a, b):   # WriteVarsToVennFiles (:329-350): (class of a, class of b), 0 none / 1 "and" / 2 "not"
    if case == "AgreedOnAlternate":
        return 1, 1
    if case in ("OneReferenceOneAlternate", "CanNotCombine"):
        return (2 if a is not None and a["type"] != "Reference" else 0), (2 if b is not None and b["type"] != "Reference" else 0)
    return 0, 0


def consensus(rows_a, rows_b, options=None, taken=None):
    """DoPairwiseVenn (:100-276) over the rows of one chromosome.  Returns (consensus rows, Venn classes of A's rows, of B's rows); a
    consensus row also holds row_a / row_b (indices, -1 = absent; the first pair's for a merged reference)."""
    o = options if options is not None else default_options()
    taken = taken if taken is not None else set()
    pool_a, pool_b = copy.deepcopy(list(rows_a)), copy.deepcopy(list(rows_b))
    for pool in (pool_a, pool_b):
        for i, v in enumerate(pool):
            v["_index"] = i
            if i and v["position"] < pool[i - 1]["position"]:
                raise ValueError("Vcf needs to be ordered.")
    venn_a, venn_b = [0] * len(pool_a), [0] * len(pool_b)
    out = []
    ia = ib = 0
    while ia < len(pool_a) or ib < len(pool_b):
        if ia < len(pool_a) and ib < len(pool_b):
            position = min(pool_a[ia]["position"], pool_b[ib]["position"])
        else:
            position = pool_a[ia]["position"] if ia < len(pool_a) else pool_b[ib]["position"]
        co_a, co_b = [], []
        while ia < len(pool_a) and pool_a[ia]["position"] == position:
            co_a.append(pool_a[ia]); ia += 1
        while ib < len(pool_b) and pool_b[ib]["position"] == position:
            co_b.append(pool_b[ib]); ib += 1
        if len(co_a) > 1 or len(co_b) > 1:
            taken.add("multi-allelic")
        if len(co_a) == 1 and co_a[0]["alt"] == "." and len(co_b) > 1:
            taken.add("pairs:ref-a-with-%d" % min(len(co_b), 3))
        if not (len(co_a) == 1 and co_a[0]["alt"] == ".") and len(co_b) == 1 and co_b[0]["alt"] == "." and len(co_a) > 1:
            taken.add("pairs:ref-b-with-%d" % min(len(co_a), 3))
        last_reference = None
        n_before = len(out)
        pairs = select_pairs(co_a, co_b)
        if len(co_a) > 1 and len(co_b) > 1 and any(a is not None and b is not None for a, b in pairs) and any(a is None or b is None for a, b in pairs):
            taken.add("pairs:partial-agreement")
        for a, b in pairs:
            case = comparison_case(a, b)
            ka, kb = venn_classes(case, a, b)
            if a is not None and ka:
                venn_a[a["_index"]] = ka
            if b is not None and kb:
                venn_b[b["_index"]] = kb
            c = combine_variants(a, b, case, o, taken)
            c["row_a"], c["row_b"] = (a["_index"] if a is not None else -1), (b["_index"] if b is not None else -1)
            if c["type"] in ("Insertion", "Deletion", "Mnv"):
                taken.add("allele:" + c["type"])
            if case == "OneReferenceOneAlternate" and (a["type"] == "Deletion" or b["type"] == "Deletion"):
                taken.add("deletion-against-reference")
            if c["genotype"] == "HomozygousRef":   # :209-243
                if last_reference is None:
                    last_reference = c
                else:
                    taken.add("reference-merge")
                    last_reference["filters"] |= c["filters"]
                    last_reference["sb"] = math_max(last_reference["sb"], c["sb"])
                    last_reference["pb_gatk"] = max(last_reference["pb_gatk"], c["pb_gatk"])
                    last_reference["pb_score"] = 0.0   # a new BiasResults
                    last_reference["noise_level"] = min(last_reference["noise_level"], c["noise_level"])
                    last_reference["genotype_qscore"] = min(last_reference["genotype_qscore"], c["genotype_qscore"])
                    last_reference["variant_qscore"] = min(last_reference["variant_qscore"], c["genotype_qscore"])
                    continue
            out.append(c)
        assert len(out) >= n_before
    return out, venn_a, venn_b
