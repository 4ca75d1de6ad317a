"""PloidyModel.DiploidByAdaptiveGT known answers of the reference's tests as data:  python tests/golden/extract_adaptive_cases.py <reference tree>
 -> tests/golden/adaptive_cases.json
  * qscores: the three tables of src/test/Pisces.Genotyping.Tests/AdaptiveGenotyperQualityCalculatorTests.cs:27-43 (truth from R; means
    {0.015, 0.5, 0.99}, priors {0.99, 0.005, 0.005}, depth 100; the harness :126-136 makes AlleleSupport = (int)(depth * frequency), for the
    hom-ref table (int)(depth * (1 - frequency)) on a Reference allele);
  * multi_allelic: GetMultiAllelicQScores :108-118 (two SNVs, depth 30, support 12 and 11: the fifth posterior is the smallest);
  * scenarios: every ExecuteAdaptiveGenotyperTest(...) of DiploidAdaptiveGenotyperTests.cs:64-110 (expected genotype of every allele, number
    of alleles to prune, reference frequency, variant frequencies, coverage; harness :20-61: a Reference row first, supports (int)(float
    frequency * coverage), MinDepthToGenotype 100, GQ range 0..100, default AdaptiveGenotypingParameters);
  * model: the SNV and indel means / priors of src/test/AdaptiveGenotyper.Tests/TestData/example.model;
  * recal_rows: the two 1/2 rows of TestData/MultiAllelicVariantTest.recal.vcf (allele types from REF / ALT, AD, DP, GQ, GP);
  * vcf_gp: the crushed 1/2 line with GP of src/test/Pisces.IO.Tests/UnitTests/VcfFileWriterTests.cs:381-443 (writer settings, the two alleles, the line)."""
import json
import os
import re
import sys


def nums(s):
    return [float(x.rstrip("f")) for x in re.findall(r"[-+]?\d*\.?\d+f?", s)] if s.strip() else []


def main(root):
    t = os.path.join(root, "src/test")
    src = open(os.path.join(t, "Pisces.Genotyping.Tests/AdaptiveGenotyperQualityCalculatorTests.cs"), encoding="utf-8-sig").read()
    means = nums(re.search(r"Means = new double\[\] \{([^}]*)\}", src).group(1))
    priors = nums(re.search(r"Priors = new double\[\] \{([^}]*)\}", src).group(1))
    body = src[src.index("public void ComputeGenotypeQualityTests()"):src.index("/* TODO")]
    depth = float(re.search(r"double depth = (\d+);", body).group(1))
    tables = []
    freqs = exp = is_ref = None
    for line in body.splitlines():
        m = re.search(r"CreatePassingVariant\((true|false)\)", line)
        if m:
            is_ref = m.group(1) == "true"
        m = re.search(r"testFrequencies = new double\[\] \{([^}]*)\}", line)
        if m:
            freqs = nums(m.group(1))
        m = re.search(r"expectedResults = new int\[\] \{([^}]*)\}", line)
        if m:
            exp = [int(x) for x in re.findall(r"\d+", m.group(1))]
        m = re.search(r"variant\.Genotype = Genotype\.(\w+);", line)
        if m:
            tables.append({"genotype": m.group(1), "reference_allele": is_ref, "depth": depth, "frequencies": freqs, "expected": exp})
    mm = re.findall(r'CreateDummyAllele\("chr1", 1000, "(\w)", "(\w)", (\d+), (\d+)\)', src)
    multi = {"alleles": [{"ref": r, "alt": a, "depth": int(d), "support": int(s)} for r, a, d, s in mm],
             "smallest_posterior_index": int(re.search(r"Assert\.Equal\((\d+), result\.GenotypePosteriors", src).group(1))}

    src = open(os.path.join(t, "Pisces.Genotyping.Tests/DiploidAdaptiveGenotyperTests.cs"), encoding="utf-8-sig").read()
    harness = {"min_depth": int(re.search(r"_minCalledVariantDepth = (\d+);", src).group(1)), "min_gq": int(re.search(r"_minGQscore = (\d+);", src).group(1)),
               "max_gq": int(re.search(r"_maxGQscore = (\d+);", src).group(1))}
    scen = []
    pat = re.compile(r"public void (\w+)\(\)\s*\{\s*ExecuteAdaptiveGenotyperTest\(Genotype\.(\w+),\s*(\d+),\s*([\d.]+)f,\s*new List<float>\s*\{([^}]*)\},"
                     r"\s*new List<FilterType>\s*\{[^}]*\},\s*(\d+)\)")
    for m in pat.finditer(src):
        scen.append({"name": m.group(1), "genotype": m.group(2), "prune": int(m.group(3)), "ref_frequency": float(m.group(4)), "alt_frequencies": nums(m.group(5)),
                     "coverage": int(m.group(6))})

    d = os.path.join(t, "AdaptiveGenotyper.Tests/TestData")
    lines = [ln.strip() for ln in open(os.path.join(d, "example.model")) if ln.strip()]
    model = {k: [float(x) for x in lines[i].split(",")] for i, k in enumerate(["snv_model", "snv_prior", "indel_model", "indel_prior"])}
    rows = []
    for ln in open(os.path.join(d, "MultiAllelicVariantTest.recal.vcf")):
        f = ln.rstrip("\n").split("\t")
        if ln.startswith("#") or len(f) < 10 or not f[9].startswith("1/2"):
            continue
        keys, vals = f[8].split(":"), f[9].split(":")
        s = dict(zip(keys, vals))
        alts = f[4].split(",")
        kind = lambda alt: "Snv" if len(alt) == len(f[3]) == 1 else "Insertion" if len(alt) > len(f[3]) else "Deletion" if len(alt) < len(f[3]) else "Mnv"
        rows.append({"position": int(f[1]), "ref": f[3], "alts": alts, "types": [kind(a) for a in alts], "ad": [int(x) for x in s["AD"].split(",")],
                     "dp": int(s["DP"]), "gq": int(s["GQ"]), "gp": s["GP"]})

    src = open(os.path.join(t, "Pisces.IO.Tests/UnitTests/VcfFileWriterTests.cs"), encoding="utf-8-sig").read()
    end = src.index("var variantLineWithGP")
    start = src.rindex("var writer = new VcfFileWriter(", 0, end)
    body = src[start:end]
    cfg = {k: v for k, v in re.findall(r"(\w+) = ([\w.]+?)f?,", body[:body.index("var candidates")])}
    alleles = []
    parts = re.split(r"new CalledAllele\(AlleleCategory\.(\w+)\)", body[body.index("var candidates"):])
    for cat, text in zip(parts[1::2], parts[2::2]):
        a = {"category": cat}
        for k, v in re.findall(r"(\w+) = ([^,\n]+),", text):
            v = v.strip()
            if k in ("AlleleSupport", "TotalCoverage", "ReferencePosition", "NumNoCalls", "ReferenceSupport", "NoiseLevelApplied"):
                a[k] = int(v)
            elif k in ("Chromosome", "ReferenceAllele", "AlternateAllele"):
                a[k] = v.strip('"')
            elif k == "Genotype":
                a[k] = v.split(".")[1]
        a["GenotypePosteriors"] = nums(re.search(r"GenotypePosteriors = new float\[\]\{([^}]*)\}", text).group(1).replace("F", ""))
        alleles.append(a)
    line = re.search(r'var variantLineWithGP = @"([^"]*)"', src).group(1)
    vcf = {"config": cfg, "alleles": alleles, "line": line}

    out = {"means": means, "priors": priors, "qscores": tables, "multi_allelic": multi, "harness": harness, "scenarios": scen, "model": model, "recal_rows": rows,
           "vcf_gp": vcf}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adaptive_cases.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    print(path, len(tables), "q-score tables,", sum(len(x["expected"]) for x in tables), "q-scores,", len(scen), "scenarios,", len(rows), "1/2 rows,", len(alleles), "VCF alleles")


if __name__ == "__main__":
    main(sys.argv[1])
