"""Writes tests/golden/venn_cases.json and venn_vcf_rows.json.gz from the reference's VennVcf test data (README_venn.md has the sources).

    python tests/golden/extract_venn_cases.py <reference root>

Data only: the body lines of the input and expected VCFs as numbers and strings (picked by field count: the expected files carry a
command-line line of their own), the options the reference's tests set, and the facts VennProcessorTests / ConsensusBuilderTests assert,
transcribed.  A line with a multi-allelic ALT (a crushed line) cannot become one row and is left out by name; more than one line in twenty
of a file left out fails the extraction."""
import gzip
import json
import os
import sys

DATA = "src/test/VennVcf.Tests/TestData"
# pair name -> pool A, pool B, expected consensus (None: asserted facts only), the options its test sets, the four Venn files
MF = {"min_frequency": 0.01, "min_frequency_filter": 0.03}
PAIRS = {
    # VennProcessorTests.cs:24-54 (debug mode: VF0..DP1)
    "control": {"a": "control_S15.vcf", "b": "control_S18.vcf", "expected": "ExpectedConsensus.vcf", "options": MF, "debug": True},
    # :57-89: VennVcfOptions as constructed, Validate() not run: MinimumFrequencyFilter is still -1 (unset).  No frequency is below -1 and none is
    # below 0, so 0 states the same
    "GRCH37": {"a": "GRCH37_S25.bam.genome.vcf", "b": "GRCH37_S30.bam.genome.vcf", "expected": "Expected_GRCH37_Consensus.vcf",
               "options": {"min_frequency_filter": 0.0}, "debug": True,
               "venn": {"a_and_b": "Expected_GRCH37_S25.bam_and_GRCH37_S30.bam.vcf", "a_not_b": "Expected_GRCH37_S25.bam_not_GRCH37_S30.bam.vcf",
                        "b_and_a": "Expected_GRCH37_S30.bam_and_GRCH37_S25.bam.vcf", "b_not_a": "Expected_GRCH37_S30.bam_not_GRCH37_S25.bam.vcf"}},
    # :113-146
    "gtTests": {"a": "gtTests_S15.vcf", "b": "gtTests_S18.vcf", "expected": "gtConsensus.vcf", "options": MF, "debug": False},
    # :671-718 (MinimumFrequencyFilter alone is set)
    "C64": {"a": "C64-Ct-4_S17.genome.vcf", "b": "C64-Ct-4_S18.genome.vcf", "expected": "ExpectedConsensus2.vcf", "options": {"min_frequency_filter": 0.03},
            "debug": False},
    # :150-251, :254-416, :419-559: asserted facts, no expected file
    "small": {"a": "small_S14.genome.vcf", "b": "small_S17.genome.vcf", "expected": None, "options": MF},
    "09H": {"a": "09H-03403-MT1-1_S7.genome.vcf", "b": "09H-03403-MT1-1_S8.genome.vcf", "expected": None, "options": MF},
    "RulesEandF": {"a": "RulesEandF_S1.genome.vcf", "b": "RulesEandF_S2.genome.vcf", "expected": None, "options": MF},
    # :92-110
    "Empty": {"a": "Empty_S1.vcf", "b": "Empty_S2.vcf", "expected": None, "options": MF},
}


def vcf_rows(path, left_out):
    rows, body = [], 0
    for number, raw in enumerate(open(path, "rb").read().decode("utf-8", errors="replace").splitlines(), 1):
        f = raw.split("\t")
        if len(f) < 10 or f[0].lstrip("\ufeff").startswith("#"):
            continue
        body += 1
        if "," in f[4]:
            left_out.append(f"{os.path.basename(path)}:{number}")
            continue
        info = dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv)
        rows.append({"line": number, "chrom": f[0], "pos": int(f[1]), "ref": f[3], "alt": f[4], "qual": f[5], "filter": f[6], "dp": int(info["DP"]),
                     "sample": dict(zip(f[8].split(":"), f[9].split(":")))})
    if (body - len(rows)) * 20 > body:
        raise SystemExit(f"{path}: {body - len(rows)} of {body} body lines cannot become rows")
    return rows


def allele(ref, alt, cat, coverage, support, gt, ref_support=0):
    return {"ref": ref, "alt": alt, "category": cat, "total_coverage": coverage, "allele_support": support, "reference_support": ref_support, "genotype": gt}


def simple_combinations(alleles, table):
    return {"alleles": alleles, "checks": [{"a": a, "b": b, "genotype": gt, "alt": alleles[alt_of]["alt"], "case": case} for a, b, gt, alt_of, case in table]}


def unit_cases():
    snv = lambda gt: allele("A", "T", "Snv", 100, 25, gt)
    ref = lambda gt, cov=100, sup=25: allele("A", ".", "Reference", cov, sup, gt, sup)
    haploid = {"hemiAltA": snv("HemizygousAlt"), "hemiAltB": snv("HemizygousAlt"), "hemiRefA": ref("HemizygousRef"), "hemiRefB": ref("HemizygousRef"),
               "hemiNoCallA": ref("HemizygousNoCall"), "hemiNoCallB": ref("HemizygousNoCall"), "NormalAltA": snv("HeterozygousAltRef"),
               "NormalRefA": ref("HomozygousRef", 300, 50)}
    half = {"AltAndNocallA": snv("AltAndNoCall"), "AltAndNocallB": snv("AltAndNoCall"), "RefAndNoCallA": ref("RefAndNoCall"), "RefAndNocallB": ref("RefAndNoCall"),
            "NocallA": ref("RefLikeNoCall"), "NoCallB": ref("RefLikeNoCall"), "NormalAltA": snv("HeterozygousAltRef"), "NormalRefA": ref("HomozygousRef", 300, 50)}
    # the two q-score tests' alleles (VennProcessorTests.cs:566-600, 727-763)
    var_a = dict(allele("A", "G", "Snv", 3067, 54, "HeterozygousAltRef", 3005), position=41266161, variant_qscore=30, genotype_qscore=30, noise_level=35, sb_gatk=-100.0)
    var_b = dict(allele("A", ".", "Reference", 3795, 3780, "HomozygousRef", 3780), position=41266161, variant_qscore=75, genotype_qscore=75, noise_level=35, sb_gatk=-100.0)
    return {
        # ConsensusBuilderTests.cs:19-128 / :130-238: VennVcfOptions' defaults after Validate(); every check runs A+B, B+A, A+null, null+B (:240-282)
        "CombineHaploidCalls": simple_combinations(haploid, [
            ("hemiAltA", "hemiAltB", "HomozygousAlt", "hemiAltA", "AgreedOnAlternate"), ("hemiRefA", "hemiRefB", "HomozygousRef", "hemiRefA", "AgreedOnReference"),
            ("hemiNoCallA", "hemiNoCallB", "RefLikeNoCall", "hemiNoCallA", "AgreedOnReference"),
            ("hemiAltA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "AgreedOnAlternate"),
            ("hemiRefA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "OneReferenceOneAlternate"),
            ("hemiNoCallA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "OneReferenceOneAlternate"),
            ("hemiAltA", "NormalRefA", "HeterozygousAltRef", "hemiAltA", "OneReferenceOneAlternate"),
            ("hemiRefA", "NormalRefA", "HomozygousRef", "NormalRefA", "AgreedOnReference"),
            ("hemiNoCallA", "NormalRefA", "HomozygousRef", "NormalRefA", "AgreedOnReference")]),
        "CombineHalfCallHalfNoCalls": simple_combinations(half, [
            ("AltAndNocallA", "AltAndNocallB", "HomozygousAlt", "AltAndNocallB", "AgreedOnAlternate"),
            ("RefAndNoCallA", "RefAndNocallB", "HomozygousRef", "RefAndNocallB", "AgreedOnReference"), ("NocallA", "NoCallB", "RefLikeNoCall", "NocallA", "AgreedOnReference"),
            ("AltAndNocallA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "AgreedOnAlternate"),
            ("RefAndNoCallA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "OneReferenceOneAlternate"),
            ("NocallA", "NormalAltA", "HeterozygousAltRef", "NormalAltA", "OneReferenceOneAlternate"),
            ("AltAndNocallA", "NormalRefA", "HeterozygousAltRef", "AltAndNocallA", "OneReferenceOneAlternate"),
            ("RefAndNoCallA", "NormalRefA", "HomozygousRef", "NormalRefA", "AgreedOnReference"), ("NocallA", "NormalRefA", "HomozygousRef", "NormalRefA", "AgreedOnReference")]),
        # VennProcessorTests.cs:561-632: TakeMin, inputs 30 and 75 -> 100
        "Qscore_Test": {"a": var_a, "b": var_b, "options": dict(MF, pool_bias_threshold=0.5, combine_qscore_method=1),
                        "expected": {"variant_qscore": 100, "genotype_qscore": 100, "ref": "A", "alt": ".", "genotype": "HomozygousRef", "allele_support": 6785,
                                     "reference_support": 6785, "total_coverage": 6862, "frequency": [0.98877, 4], "noise_level": 35, "sb_gatk": -100, "pb_gatk": -100}},
        # :723-840: one pair of objects through six calls; a call's rewritten VariantQscore stays with the object
        "Qscore_DiffentNL_Test": {"a": var_a, "b": dict(var_b, noise_level=2), "options": dict(MF, pool_bias_threshold=0.5), "steps": [
            {"method": 0, "members": "ab", "expected": {"variant_qscore": 100, "ref": "A", "alt": ".", "genotype": "HomozygousRef", "total_coverage": 6862, "reference_support": 6785,
                                                         "allele_support": 6785, "genotype_qscore": 100, "frequency": [0.98877877, 6], "noise_level": 5, "sb_gatk": -100, "pb_gatk": -100}},
            {"method": 1, "members": "ab", "expected": {"noise_level": 2, "variant_qscore": 100}},
            {"method": 1, "members": "a", "expected": {"noise_level": 35, "variant_qscore": 100}},
            {"method": 1, "members": "b", "expected": {"noise_level": 2, "variant_qscore": 100}},
            {"method": 0, "members": "a", "expected": {"noise_level": 35, "variant_qscore": 100}},
            {"method": 0, "members": "b", "expected": {"noise_level": 2, "variant_qscore": 100}}]},
    }


def assertions():
    v = lambda gt, freq, q, filters, **more: dict({"genotype": gt, "frequency": [freq, 4], "variant_qscore": q, "filters": filters}, **more)
    return {
        # VennProcessorTests.cs:203-248: consensus rows by index, the four Venn files as (position, ref, alt)
        "small": {"consensus": {"3": {"frequency": [0.8558, 4], "filters": ["PoolBias"], "ref": "A", "alt": "."},
                                "6": {"pos": 115258744, "frequency": [0.8711, 4], "filters": [], "ref": "C", "alt": "."}},
                  "venn": {"a_and_b": [[115258743, "AC", "TT"], [115258747, "C", "T"]], "b_and_a": [[115258743, "AC", "TT"], [115258747, "C", "T"]],
                           "a_not_b": [[115258743, "A", "T"], [115258744, "C", "T"]], "b_not_a": []}},
        # :273-414: PoolAVariants[i] with PoolBVariants[i] through CombineVariants, rules A, B, C-a, C-b, D
        "09H": [
            {"index": 0, "a": v("HomozygousRef", 0.9979, 100, []), "b": v("HeterozygousAltRef", 0.0173, 100, []), "case": "OneReferenceOneAlternate",
             "consensus": v("HomozygousRef", 0.9907, 100, [])},
            {"index": 1, "a": v("HeterozygousAltRef", 0.0776, 100, []), "b": v("HomozygousRef", 0.9989, 100, []), "case": "OneReferenceOneAlternate",
             "consensus": v("AltLikeNoCall", 0.0070, 0, ["PoolBias"])},
            {"index": 2, "a": v("HeterozygousAltRef", 0.0367, 100, []), "b": v("HomozygousRef", 0.9976, 100, []), "case": "OneReferenceOneAlternate",
             "consensus": v("AltLikeNoCall", 0.0117, 23, ["PoolBias"])},
            {"index": 3, "a": v("HeterozygousAltRef", 0.01725, 100, []), "b": v("HeterozygousAltRef", 0.03667, 100, []), "case": "AgreedOnAlternate",
             "consensus": v("AltLikeNoCall", 0.02347, 100, [])},
            {"index": 4, "a": v("HeterozygousAltRef", 0.2509, 100, []), "b": v("HeterozygousAltRef", 0.0367, 100, []), "case": "AgreedOnAlternate",
             "consensus": v("HeterozygousAltRef", 0.1716, 100, [])}],
        # :455-555: rule E (several REF calls of one position become one) and rule F (several no-calls stay apart)
        "RulesEandF": {
            "a": {"0": v("HomozygousRef", 0.9979, 100, [], pos=25378561), "1": v("HeterozygousAltRef", 0.0776, 100, [], pos=25378562),
                  "2": v("HeterozygousAltRef", 0.0776, 100, [], pos=25378562), "3": v("HeterozygousAltRef", 0.0776, 100, [], pos=25378562)},
            "b": {"0": v("HeterozygousAltRef", 0.0173, 100, [], pos=25378561), "1": v("HomozygousRef", 0.9827, 100, [], pos=25378561),
                  "2": v("HomozygousRef", 0.9989, 100, [], pos=25378562), "3": {"pos": 25378563}},
            "consensus": {"0": v("HomozygousRef", 0.9907, 100, [], pos=25378561), "1": v("AltLikeNoCall", 0.0069, 0, ["PoolBias"], pos=25378562, ref="C", alt="T"),
                          "2": {"pos": 25378562, "genotype": "AltLikeNoCall", "frequency": [0.0069, 4], "variant_qscore": 0, "ref": "C", "alt": "TT"},
                          "3": {"pos": 25378562, "genotype": "AltLikeNoCall", "frequency": [0.0069, 4], "variant_qscore": 0, "ref": "CC", "alt": "T"},
                          "4": {"pos": 25378563}}},
        # :700-716
        "C64": {"rows_at": {"chrom": "chr15", "pos": 92604460, "count": 1}},
    }


def main(root):
    data = os.path.join(root, DATA)
    names = set()
    for p in PAIRS.values():
        names |= {p["a"], p["b"]} | ({p["expected"]} if p["expected"] else set()) | set(p.get("venn", {}).values())
    left_out = []
    here = os.path.dirname(os.path.abspath(__file__))
    files = {name: vcf_rows(os.path.join(data, name), left_out) for name in sorted(names)}
    # what was transcribed by hand stays readable; the ~1000 body lines of the VCFs travel compressed (mtime 0: the same bytes every time)
    with open(os.path.join(here, "venn_cases.json"), "w") as fp:
        top = {"left_out": left_out, "pairs": PAIRS, "assertions": assertions(), "unit": unit_cases()}
        parts = []
        for key in sorted(top):   # a second-level entry a line
            inner = top[key]
            body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(inner[k], sort_keys=True)}" for k in sorted(inner)) if isinstance(inner, dict) else None
            parts.append(f" {json.dumps(key)}: " + ("{\n" + body + "\n }" if body else json.dumps(inner)))
        fp.write("{\n" + ",\n".join(parts) + "\n}\n")
    with open(os.path.join(here, "venn_vcf_rows.json.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as fp:
        fp.write(json.dumps(files, sort_keys=True, separators=(",", ":")).encode())
    print({k: len(v) for k, v in files.items()}, "left out:", left_out)


if __name__ == "__main__":
    main(sys.argv[1])
