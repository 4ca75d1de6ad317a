"""VariantQualityRecalibration stated in plain Python over dicts, for the tests of the VQR entries.  It follows the reference's files line
by line (src/exe/VariantQualityRecalibration/: MutationCategory.cs, MutationCounter.cs, CountData.cs, EdgeIssueCountData.cs,
SignatureSorter.cs, QualityRecalibration.cs) and shares no code with the library; the only thing it does not restate is
VariantQualityCalculator.AssignPoissonQScore, which is the oracle's orc_poisson_qscore.

A row is a dict: position, total_coverage, allele_support, variant_qscore, genotype_qscore, noise_level, filter_bits (bit i = FilterType
i), type ("Reference" / "Snv" / "Insertion" / "Deletion" / "Mnv"), ref and alt (strings; "." is the reference call's alt).
"""
import math

CATEGORIES = ("AtoC", "AtoG", "AtoT", "CtoA", "CtoG", "CtoT", "GtoA", "GtoC", "GtoT", "TtoA", "TtoC", "TtoG", "Insertion", "Deletion", "Reference",
              "Other")
SNV_CATEGORIES = CATEGORIES[:12]
INT_MIN = -2147483648
FILTER_LOW_VARIANT_QSCORE, FILTER_FORCED_REPORT = 3, 10
FILTER_BIT = {"SB": 0, "LowVariantQscore": 3, "q30": 3, "LowDP": 4, "LowVariantFreq": 5, "OffTarget": 11, "ForcedReport": 10}

# how often AssignPoissonQScore was asked for a Poisson tail with a noise level of int.MinValue (the device relies on: never)
INT_MIN_REACHED_POISSON = [0]


# ---- C# arithmetic ------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    a, b = float(a), float(b)
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def cs_int(d):
    """(int) of a Double: truncation; NaN, the infinities and everything out of range give int.MinValue"""
    if d != d or d in (float("inf"), float("-inf")) or not (-2147483649.0 < d < 2147483648.0):
        return INT_MIN
    return int(d)


def q_to_p(q):   # MathOperations.QtoP: Math.Pow(10, -1 * q / 10f)
    try:
        return math.pow(10.0, -1 * float(q) / 10.0)
    except OverflowError:
        return float("inf")


def p_to_q(p):   # MathOperations.PtoQ: -10 * Math.Log10(p)
    if p != p or p < 0:
        return float("nan")
    if p == 0:
        return float("inf")
    if p == float("inf"):
        return float("-inf")
    return -10 * math.log10(p)


# ---- categories ---------------------------------------------------------------------------------------------------------------------
def category_of_strings(reference_allele, alternate_allele):   # MutationCategory.cs:53-81
    if len(reference_allele) > len(alternate_allele):
        return "Deletion"
    if len(reference_allele) < len(alternate_allele):
        return "Insertion"
    if len(reference_allele) != 1 or len(alternate_allele) != 1:
        return "Other"
    if alternate_allele == "." or alternate_allele == reference_allele:
        return "Reference"
    name = (reference_allele + "to" + alternate_allele).lower()
    for c in CATEGORIES:
        if name == c.lower():
            return c
    return "Other"


def count_category(row):   # MutationCategory.cs:41-50
    if row["type"] == "Reference":
        return "Reference"
    return category_of_strings(row["ref"], row["alt"])


def update_category(row):   # MutationCounter.cs:133-172
    if row["filter_bits"] & (1 << FILTER_FORCED_REPORT):
        return "Other"
    t = row["type"]
    if t == "Reference":
        return "Reference"
    if t == "Deletion":
        return "Deletion"
    if t == "Insertion":
        return "Insertion"
    if t == "Snv":
        name = (row["ref"] + "to" + row["alt"]).lower()
        for c in CATEGORIES:
            if name == c.lower():
                return c
        return "Other"
    return "Other"


# ---- counting -----------------------------------------------------------------------------------------------------------------------
def new_counts():
    return {"by": {c: 0.0 for c in CATEGORIES}, "npv": 0.0}


def did_we_detect_an_edge(test_index, buffer):
    """EdgeIssueCountData.cs:67-118; a slot is None or (position, total_coverage) — a row of another chromosome is None here (:95)"""
    test = buffer[test_index]
    if test is None:
        return False
    if test[1] == 0:
        return False
    for i in range(len(buffer)):
        if i == test_index:
            continue
        b = buffer[i]
        if b is None:
            return True
        if b[1] < 0.5 * test[1]:
            return True
        distance = test[0] - b[0]
        max_allowed = test_index - i
        if max_allowed > 0:
            if distance > max_allowed:
                return True
        else:
            if distance < max_allowed:
                return True
    return False


def strain(rows, extent, edges=True, lo=0, hi=None, basic=None, edge=None):
    """SignatureSorter.StrainVcf (:50-82) over the rows of one chromosome: basic counts, edge counts and the suspect flag of every row.
    Rows [lo, hi) are counted; the trailing buffer sees every row (the halo of a streaming caller)."""
    hi = len(rows) if hi is None else hi
    basic = basic if basic is not None else new_counts()
    edge = edge if edge is not None else new_counts()
    suspect = [0] * len(rows)
    for i in range(lo, hi):   # CountData.Add (:59-76)
        c = count_category(rows[i])
        basic["npv"] += 1
        if c != "Reference":
            basic["by"][c] += 1
    if edges:
        length = 2 * extent + 1
        buffer = [None] * length   # (row index, position, coverage)
        for step in range(len(rows) + extent):   # the rows, then `extent` nulls (:75-76)
            nxt = None
            if step < len(rows):
                r = rows[step]
                nxt = (r["position"], r["total_coverage"], step)
            buffer = buffer[1:] + [nxt]
            if did_we_detect_an_edge(extent, buffer):
                i = buffer[extent][2]
                if not (lo <= i < hi):
                    continue
                c = category_of_strings(rows[i]["ref"], rows[i]["alt"]) if rows[i]["type"] != "Reference" else "Reference"
                edge["npv"] += 1
                if c != "Reference":
                    edge["by"][c] += 1
                    suspect[i] = 1
    return basic, edge, suspect


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def total_mutations(counts):
    t = 0.0
    for v in counts["by"].values():
        t += v
    return t


def observed_mutation_rate(counts):
    if counts["npv"] == 0:
        return 0.0
    return _div(total_mutations(counts), counts["npv"])


def phred_scaled_calibrated_rates(baseline_q_noise, z_factor, counts):   # QualityRecalibration.cs:323-381
    base_noise_rate = q_to_p(baseline_q_noise)
    by = counts["by"]
    for c in ("Deletion", "Insertion", "Other", "Reference"):
        by.pop(c, None)
    sorted_counts = sorted(by.values())
    if len(by) != 12:
        return None
    avg = 0.0
    for i in range(2, 10):
        avg += sorted_counts[i] / 8.0
    variance = 0.0
    for i in range(2, 10):
        variance += (avg - sorted_counts[i]) * (avg - sorted_counts[i]) / 8.0
    threshold = avg + z_factor * math.sqrt(variance)
    out = {}
    for c in by:
        n = by[c]
        if n > threshold:
            observed = 0.0
            if counts["npv"] > 0:
                observed = n / counts["npv"]
            out[c] = cs_int(p_to_q(observed + base_noise_rate))
    return out


def phred_scaled_calibrated_rates_for_edges(basic, edge):   # :276-321
    increase = _div(observed_mutation_rate(edge), observed_mutation_rate(basic))
    not_in_edge = total_mutations(basic) - total_mutations(edge)
    loci_not_in_edge = basic["npv"] - edge["npv"]
    rate_not_in_edge = _div(not_in_edge, loci_not_in_edge)
    expected = rate_not_in_edge * edge["npv"]
    probably_wrong = total_mutations(edge) - expected
    error_rate = _div(probably_wrong, total_mutations(edge))
    out = {}
    for c in edge["by"]:
        proportion = _div(edge["by"][c], total_mutations(edge))
        out[c] = cs_int(p_to_q(proportion * error_rate))
    return out, increase


def tables(options, basic, edge):
    """GetRecalibrationTables (:58-129) on copies of the two CountData; options is a dict with the names of PiscesVqrOptions"""
    basic = {"by": dict(basic["by"]), "npv": float(basic["npv"])}
    edge = {"by": dict(edge["by"]), "npv": float(edge["npv"])}
    if options["loci_count"] > 0:   # SignatureSorter.cs:78-82
        basic["npv"] = float(options["loci_count"])
        edge["npv"] = float(options["loci_count"])
    out = {"basic": None, "edge": None, "edge_risk": None, "general_edge_risk_increase": None}
    if options["do_basic_checks"]:
        out["basic"] = phred_scaled_calibrated_rates(options["base_q_noise"], options["z_factor"], basic)
    if options["do_amplicon_position_checks"]:
        out["edge"] = phred_scaled_calibrated_rates(options["base_q_noise"], options["z_factor"], edge)
    if options["do_basic_checks"] and options["do_amplicon_position_checks"]:
        out["edge_risk"], out["general_edge_risk_increase"] = phred_scaled_calibrated_rates_for_edges(basic, edge)
    return out


# ---- the update ---------------------------------------------------------------------------------------------------------------------
def assign_poisson_qscore(call_count, coverage, noise_level, max_qscore):   # VariantQualityCalculator.cs:54-65
    if call_count <= 0 or coverage <= 0:
        return 0
    if noise_level == INT_MIN:
        # QtoP is +inf: MathNet's Poisson(+inf).CumulativeDistribution is 0, p = 1, Q = 0 (what oracle/pisces_oracle.c says of the same
        # level under NoiseModel.Window); counted, because under subsampling this line must never be reached
        INT_MIN_REACHED_POISSON[0] += 1
        return 0
    from tests import orc
    return int(orc.lib.orc_poisson_qscore(int(call_count), int(coverage), int(noise_level), int(max_qscore)))


def have_info_to_update_q(row):   # :257-274
    if row["variant_qscore"] < 1:
        return False, -1.0, -1.0
    return True, float(row["total_coverage"]), float(row["allele_support"])


def insert_new_q(rates, row, cat, new_q, is_somatic):   # :248-255
    row["variant_qscore"] = new_q
    row["noise_level"] = rates[cat]
    row["rewritten"] = True   # (the tests' bookkeeping: what the device counts in *d_n_changed)
    if is_somatic:
        row["genotype_qscore"] = new_q


def update_variant_qscore_and_refilter(max_qscore, filter_qscore, rates, row, cat, subsample):   # :197-246
    denominator = q_to_p(rates[cat])
    sub_sample_to_this = _div(1.0, denominator)
    if rates[cat] == 0 or denominator == 0:
        subsample = False
    can_update, depth, call_count = have_info_to_update_q(row)
    if subsample and depth > sub_sample_to_this:
        call_count = call_count * sub_sample_to_this / depth
        depth = sub_sample_to_this
    if can_update:
        new_q = assign_poisson_qscore(cs_int(call_count), cs_int(depth), rates[cat], min(row["variant_qscore"], max_qscore))
        insert_new_q(rates, row, cat, new_q, True)
        if new_q < filter_qscore:
            if row["filter_bits"] & (1 << FILTER_LOW_VARIANT_QSCORE):
                return
            row["filter_bits"] |= 1 << FILTER_LOW_VARIANT_QSCORE


def update_allele(options, T, row, suspect_positions):   # :131-155; suspect_positions: AmpliconEdgeVariantsList of the row's chromosome
    cat = update_category(row)
    changed = False
    if options["do_basic_checks"] and T["basic"] is not None and cat in T["basic"]:
        update_variant_qscore_and_refilter(options["max_qscore"], options["filter_qscore"], T["basic"], row, cat, False)
        changed = True
    if options["do_amplicon_position_checks"] and T["edge"] is not None and cat in T["edge"] and row["position"] in suspect_positions:
        update_variant_qscore_and_refilter(options["max_qscore"], options["filter_qscore"], T["edge_risk"], row, cat, True)
        changed = True
    return changed


def apply(options, T, rows, suspect):
    """UpdateAllele over the rows of one chromosome, in place; suspect[i] as strain() left it"""
    positions = {rows[i]["position"] for i in range(len(rows)) if suspect is not None and suspect[i]}
    for row in rows:
        update_allele(options, T, row, positions)
    return rows


# ---- dicts <-> the library's structures (the tests' glue; nothing of the algorithm) -------------------------------------------------
DEFAULT_OPTIONS = {"do_basic_checks": 1, "do_amplicon_position_checks": 0, "extent_of_edge_region": 4, "loci_count": -1, "base_q_noise": 20,
                   "filter_qscore": 30, "max_qscore": 100, "z_factor": 2.0, "alignment_warning_threshold": 10.0}


def options(**kw):
    o = dict(DEFAULT_OPTIONS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def row_of_vcf(v):
    """a row of tests/golden/vqr_cases.json: DP is total_coverage, AD[1] allele_support, QUAL variant_qscore"""
    ref, alt = v["ref"], v["alt"]
    if alt == ".":
        t = "Reference"
    elif len(ref) == 1 and len(alt) == 1:
        t = "Snv"
    elif len(ref) > len(alt):
        t = "Deletion"
    elif len(ref) < len(alt):
        t = "Insertion"
    else:
        t = "Mnv"
    bits = 0
    for name in v["filter"].split(";"):
        if name not in ("PASS", "."):
            bits |= 1 << FILTER_BIT[name]
    return {"position": v["pos"], "total_coverage": v["dp"], "allele_support": v["ad"][1] if len(v["ad"]) > 1 else v["ad"][0], "variant_qscore": v["qual"],
            "genotype_qscore": v["gq"], "noise_level": v["nl"], "filter_bits": bits, "type": t, "ref": ref, "alt": alt}


def records_of_rows(rows):
    import numpy as np
    from pisces_amd import _abi
    cat = {"Snv": _abi.CAT_SNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION, "Mnv": _abi.CAT_MNV, "Reference": _abi.CAT_REFERENCE}
    recs = np.zeros(len(rows), dtype=_abi.CALLED_ALLELE_DTYPE)
    for i, r in enumerate(rows):
        single = r["type"] in ("Snv", "Reference")
        rc = _abi.ALLELE_OF_BASE.get(r["ref"][:1].upper(), _abi.ALLELE_N)
        ac = _abi.ALLELE_OF_BASE.get(r["alt"].upper(), _abi.ALLELE_N) if (single and r["alt"] != ".") else (rc if r["type"] == "Reference" else _abi.ALLELE_N)
        recs[i]["position"] = r["position"]
        recs[i]["total_coverage"] = r["total_coverage"]
        recs[i]["allele_support"] = r["allele_support"]
        recs[i]["reference_support"] = max(0, r["total_coverage"] - r["allele_support"])
        recs[i]["variant_qscore"] = r["variant_qscore"]
        recs[i]["genotype_qscore"] = r["genotype_qscore"]
        recs[i]["noise_level"] = -32768 if r["noise_level"] == INT_MIN else r["noise_level"]
        recs[i]["filter_bits"] = r["filter_bits"]
        recs[i]["info"] = 2 | (cat[r["type"]] << 4) | (rc << 7) | (ac << 10)   # genotype 0/1 (HET_ALT_REF = 2)
    return recs


def rows_of_records(recs):
    """records the caller made (Reference / SNV rows: the alleles are the base codes of `info`) as the statement's dicts"""
    from pisces_amd import _abi
    names = {_abi.CAT_SNV: "Snv", _abi.CAT_INSERTION: "Insertion", _abi.CAT_DELETION: "Deletion", _abi.CAT_MNV: "Mnv", _abi.CAT_REFERENCE: "Reference"}
    rows = []
    for r in recs:
        info = int(r["info"])
        t = names[(info >> 4) & 7]
        assert t in ("Snv", "Reference"), t
        ref = _abi.BASE_OF_ALLELE[(info >> 7) & 7]
        alt = "." if t == "Reference" else _abi.BASE_OF_ALLELE[(info >> 10) & 7]
        nl = int(r["noise_level"])
        rows.append({"position": int(r["position"]), "total_coverage": int(r["total_coverage"]), "allele_support": int(r["allele_support"]),
                     "variant_qscore": int(r["variant_qscore"]), "genotype_qscore": int(r["genotype_qscore"]),
                     "noise_level": INT_MIN if nl == -32768 else nl, "filter_bits": int(r["filter_bits"]), "type": t, "ref": ref, "alt": alt})
    return rows


def write_back(recs, rows):
    """the four fields an update writes, from the statement's rows onto a copy of the records"""
    out = recs.copy()
    for i, (q, gq, nl, bits) in enumerate(fields_of_rows(rows)):
        out[i]["variant_qscore"], out[i]["genotype_qscore"], out[i]["noise_level"], out[i]["filter_bits"] = q, gq, nl, bits
    return out


def fields_of_rows(rows):
    """(variant_qscore, genotype_qscore, noise_level as the record holds it, filter_bits) of every row"""
    return [(r["variant_qscore"], r["genotype_qscore"], -32768 if r["noise_level"] == INT_MIN else r["noise_level"], r["filter_bits"]) for r in rows]


def counts_pair(basic, edge):
    """two statement CountData as ((by_category[16], num_possible), ...) for engine.vqr_counts_array"""
    return [([int(c["by"].get(k, 0)) for k in CATEGORIES], int(c["npv"])) for c in (basic, edge)]


def counts_of_struct(arr):
    return [([int(x) for x in arr[k].by_category], int(arr[k].num_possible_variants)) for k in range(2)]


def tables_of_struct(t):
    """a PiscesVqrTables as the statement's dict of dicts"""
    def table(values, mask):
        return {SNV_CATEGORIES[c]: int(values[c]) for c in range(12) if (mask >> c) & 1}
    return {"basic": table(t.basic, t.basic_mask), "edge": table(t.edge, t.edge_mask),
            "edge_risk": table(t.edge_risk, 0xfff) if t.has_edge_risk else None, "general_edge_risk_increase": t.general_edge_risk_increase}


def struct_of_tables(T):
    from pisces_amd import _abi
    t = _abi.PiscesVqrTables()
    for name, mask in (("basic", "basic_mask"), ("edge", "edge_mask")):
        m = 0
        for c, k in enumerate(SNV_CATEGORIES):
            if T.get(name) and k in T[name]:
                getattr(t, name)[c] = T[name][k]
                m |= 1 << c
        setattr(t, mask, m)
    if T.get("edge_risk") is not None:
        for c, k in enumerate(SNV_CATEGORIES):
            t.edge_risk[c] = T["edge_risk"][k]
        t.has_edge_risk = 1
    return t
