"""Rows for the VennVcf tests (tests/test_venn_cpu.py, tests/test_venn_gpu.py): the goldens of tests/golden/venn_cases.json mapped to the
statement's dicts (tests/venn_ref.py) the way AlleleReader maps a VCF line, the dicts mapped to the library's 64-byte rows and back, and
seeded pairs of row sets in which every branch of the consensus is drawn often."""
import gzip
import json
import os

import numpy as np

from pisces_amd import _abi
from tests import venn_ref as R

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = json.load(open(os.path.join(_HERE, "venn_cases.json")))
GOLDEN["files"] = json.loads(gzip.open(os.path.join(_HERE, "venn_vcf_rows.json.gz")).read())   # the VCFs' body lines (README_venn.md)
CODE_OF_BASE = {"A": 0, "G": 1, "C": 2, "T": 3, "N": 4}


def map_gt_string(gt, num_alts):   # VcfVariantUtilities.MapGTString (VcfVariantUtilities.cs:503-545)
    gt = gt.replace("|", "/")
    table = {"1/1": "HomozygousAlt", "0/0": "HomozygousRef", "./1": "AltAndNoCall", "1/.": "AltAndNoCall", "./0": "RefAndNoCall", "0/.": "RefAndNoCall",
             "1/0": "HeterozygousAltRef", "0/1": "HeterozygousAltRef", "2/1": "HeterozygousAlt1Alt2", "1/2": "HeterozygousAlt1Alt2", ".": "HemizygousNoCall",
             "0": "HemizygousRef", "1": "HemizygousAlt", "*/*": "Others", "2/2": "Others"}
    if gt == "./.":
        return ("RefLikeNoCall", "AltLikeNoCall")[num_alts] if num_alts < 2 else "Alt12LikeNoCall"
    return table.get(gt, "RefLikeNoCall")


GT_STRING = {"HomozygousAlt": "1/1", "HomozygousRef": "0/0", "HeterozygousAltRef": "0/1", "RefLikeNoCall": "./.", "AltLikeNoCall": "./.",
             "HeterozygousAlt1Alt2": "1/2", "Alt12LikeNoCall": "./.", "AltAndNoCall": "1/.", "RefAndNoCall": "0/.", "HemizygousRef": "0", "HemizygousAlt": "1",
             "HemizygousNoCall": "."}


def map_filter_string(raw):   # VcfVariantUtilities.MapFilterString (:404-472), bit i = FilterType i
    s = (raw or "").strip()
    if s in (".", "") or s.lower() == "pass":
        return 0
    bits = 0
    for f in s.lower().split(";"):
        f = f.strip()
        if f in (".", ""):
            continue
        try:
            threshold = int(f[1:])
        except ValueError:
            threshold = -1
        if "lowq" in f or (f[0] == "q" and threshold > 0):
            bits |= 1 << 3
        elif f == "pb":
            bits |= 1 << 1
        elif f == "sb":
            bits |= 1 << 0
        elif f == "ab":
            bits |= 1 << 2
        elif f in ("lowdp", "lowdepth"):
            bits |= 1 << 4
        elif f in ("lowvariantfreq", "lowfreq"):
            bits |= 1 << 5
        elif f == "lowgq" or f[:2] == "gq":
            bits |= 1 << 6
        elif f[0] == "r" and threshold > 0:
            bits |= 1 << 7
        elif f[0] == "r" and len(f[1:].split("x")) == 2 and all(p.lstrip("-").isdigit() for p in f[1:].split("x")):
            bits |= 1 << 9
        elif f == "multiallelicsite":
            bits |= 1 << 8
        elif f == "forcedreport":
            bits |= 1 << 10
        elif f == "nc":
            bits |= 1 << 12
        else:
            raise ValueError(f"filter {f!r}: FilterType.Unknown has no bit in a row")
    return bits


def row_of_line(line):
    """AlleleReader.AssignVariantInfo (AlleleReader.cs:96-250) for an uncrushed one-allele line, in its order: DP, AD[0], AD[1] (a reference
    line: both supports from the single AD), QUAL, GQ, NL, GT, FILTER, SB."""
    sample = line["sample"]
    is_ref = line["alt"] == "."
    ad = sample.get("AD", "0,0").split(",")
    reference_support = int(ad[0])
    alt_support = int(ad[1]) if not is_ref and len(ad) > 1 else 0
    sb_gatk = float(np.float32(sample["SB"])) if "SB" in sample else -100.0
    return {"chrom": line["chrom"], "position": line["pos"], "ref": line["ref"], "alt": line["alt"], "type": R.set_type(line["ref"], line["alt"]),
            "total_coverage": line["dp"], "reference_support": reference_support, "allele_support": reference_support if is_ref else alt_support,
            "variant_qscore": int(float(line["qual"])), "genotype_qscore": int(sample["GQ"]) if "GQ" in sample else 0, "noise_level": int(sample.get("NL", 0)),
            "genotype": map_gt_string(sample.get("GT", ""), 0 if is_ref else 1), "filters": map_filter_string(line["filter"]),
            "sb": 10.0 ** (sb_gatk / 10.0)}


def rows_of_file(name):
    return [row_of_line(line) for line in GOLDEN["files"][name]]


def chromosomes(*row_lists):
    """chromosome names in order of first appearance over the lists"""
    seen = []
    for rows in row_lists:
        for r in rows:
            if r["chrom"] not in seen:
                seen.append(r["chrom"])
    return seen


def options_of(overrides):
    return R.default_options(**overrides)


# ---- the statement's dicts <-> the library's rows -------------------------------------------------------------------------------------
def record_of(d):
    """(CALLED_ALLELE_DTYPE row, (ref, alt) pair) of a statement dict"""
    r = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)[0]
    for k in ("position", "total_coverage", "allele_support", "reference_support", "variant_qscore", "genotype_qscore"):
        r[k] = d[k]
    r["num_no_calls"] = d.get("num_no_calls", 0)
    r["coverage_by_dir"] = d.get("coverage_by_dir", [0, 0, 0])
    r["support_by_dir"] = d.get("support_by_dir", [0, 0, 0])
    r["noise_level"] = -32768 if d["noise_level"] == R.INT_MIN else d["noise_level"]
    r["strand_bias_score"] = d["sb"]
    r["filter_bits"] = d["filters"]
    single = len(d["ref"]) == 1 and len(d["alt"]) == 1
    ref_code = CODE_OF_BASE.get(d["ref"][0].upper(), 4)
    if d["type"] == "Reference":
        alt_code = ref_code
    elif single:
        alt_code = CODE_OF_BASE.get(d["alt"].upper(), 4)
    else:
        alt_code = 4
    r["info"] = R.GENOTYPES.index(d["genotype"]) | (R.TYPES.index(d["type"]) << 4) | (ref_code << 7) | (alt_code << 10) | (d.get("bias_bits", 0) << 13)
    return r, (d["ref"], d["alt"])


def records_of(dicts):
    pairs = [record_of(d) for d in dicts]
    recs = np.array([p[0] for p in pairs], dtype=_abi.CALLED_ALLELE_DTYPE) if pairs else np.zeros(0, dtype=_abi.CALLED_ALLELE_DTYPE)
    return recs, [p[1] for p in pairs]


def options_struct(o):
    from pisces_amd import engine
    return engine.venn_options(**o)


def dicts_of(result):
    """the statement's view of what engine.venn_consensus (or the device path, gathered into the same dict) returned"""
    out = []
    for rec, (ref, alt), info in zip(result["records"], result["alleles"], result["info"]):
        word = int(rec["info"])
        level = int(rec["noise_level"])
        out.append({"position": int(rec["position"]), "ref": ref, "alt": alt, "type": R.TYPES[(word >> 4) & 7], "genotype": R.GENOTYPES[word & 15],
                    "total_coverage": int(rec["total_coverage"]), "allele_support": int(rec["allele_support"]), "reference_support": int(rec["reference_support"]),
                    "variant_qscore": int(rec["variant_qscore"]), "genotype_qscore": int(rec["genotype_qscore"]), "noise_level": R.INT_MIN if level == -32768 else level,
                    "filters": int(rec["filter_bits"]), "sb": float(rec["strand_bias_score"]), "num_no_calls": int(rec["num_no_calls"]),
                    "coverage_by_dir": [int(x) for x in rec["coverage_by_dir"]], "support_by_dir": [int(x) for x in rec["support_by_dir"]], "bias_bits": word >> 13,
                    "case": R.CASES[int(info["comparison_case"])], "alt_changed_to_ref": bool(info["alt_changed_to_ref"]), "pb_score": float(info["pool_bias_score"]),
                    "pb_gatk": float(info["pool_bias_gatk"]), "row_a": int(info["row_a"]), "row_b": int(info["row_b"])})
    return out


EXACT_FIELDS = ("position", "ref", "alt", "type", "genotype", "total_coverage", "allele_support", "reference_support", "variant_qscore", "genotype_qscore",
                "noise_level", "filters", "num_no_calls", "coverage_by_dir", "support_by_dir", "bias_bits", "case", "alt_changed_to_ref", "row_a", "row_b")


def assert_same_consensus(got, want, where=""):
    """library rows (dicts_of) against the statement's: every field exactly, the two pool-bias scores at the project's rtol for the
    strand-bias score (tests/test_gpu_parity.py: 1e-9), the strand-bias score itself bit for bit (it is copied)"""
    assert len(got) == len(want), (where, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for k in EXACT_FIELDS:
            assert g[k] == w[k], (where, i, k, g[k], w[k], w)
        assert g["sb"] == w["sb"] or (g["sb"] != g["sb"] and w["sb"] != w["sb"]), (where, i, "sb", g["sb"], w["sb"])
        for k in ("pb_score", "pb_gatk"):
            assert np.isclose(g[k], w[k], rtol=1e-9, atol=0.0) or g[k] == w[k], (where, i, k, g[k], w[k], w)


# ---- a consensus row as the VCF line VennVcfWriter writes, field by field ---------------------------------------------------------------
def line_fields(c, rows_a, rows_b):
    is_ref = c["type"] == "Reference"
    depth = max(c["reference_support"] if is_ref else c["reference_support"] + c["allele_support"], c["total_coverage"], c["allele_support"])   # GetDepthCountInt
    # VcfFileWriter.WriteListOfColocatedAlleles (VcfFileWriter.cs:234-244): a reference-like genotype is written with ALT "."
    alt = "." if c["genotype"] in ("HomozygousRef", "RefLikeNoCall", "RefAndNoCall", "HemizygousNoCall", "HemizygousRef") and not (c["filters"] >> 10) & 1 else c["alt"]
    f = {"pos": c["position"], "ref": c["ref"], "alt": alt, "qual": c["variant_qscore"], "filter": c["filters"], "dp": depth,
         "GT": GT_STRING[c["genotype"]], "GQ": c["genotype_qscore"], "AD": [c["reference_support"]] if is_ref else [c["reference_support"], c["allele_support"]],
         "NL": c["noise_level"], "PB": min(max(c["pb_gatk"], -100.0), 0.0)}
    for k, (rows, i) in enumerate(((rows_a, c["row_a"]), (rows_b, c["row_b"]))):
        f[f"AD{k}"] = "NA" if i < 0 else rows[i]["allele_support"]
        f[f"DP{k}"] = "NA" if i < 0 else rows[i]["total_coverage"]
    return f


def written_order(consensus_rows):
    """VennVcfWriter.Write (VennVcfWriter.cs:106-107) orders what it is handed by locus, then ReferenceAllele, then AlternateAllele (the
    object's strings, a stable sort): the order of an expected file's lines, not of the consensus rows"""
    return sorted(consensus_rows, key=lambda c: (c["position"], c["ref"], c["alt"]))


def assert_line(c, rows_a, rows_b, line, debug, where):
    """QUAL, FILTER, DP, GT, GQ, AD, NL, PB — and VF0..DP1 where the expected file has them — of one expected body line.  PB: |difference| <=
    5e-5 + 1e-9, the half-unit of the file's four decimals plus slack far above a few ulp of a double near 100."""
    f = line_fields(c, rows_a, rows_b)
    s = line["sample"]
    assert (f["pos"], f["ref"], f["alt"]) == (line["pos"], line["ref"], line["alt"]), (where, f, line)
    assert f["qual"] == int(float(line["qual"])), (where, "QUAL", f, line)
    assert f["filter"] == map_filter_string(line["filter"]), (where, "FILTER", f, line)
    assert f["dp"] == line["dp"], (where, "DP", f, line)
    assert f["GT"] == s["GT"] and f["GQ"] == int(s["GQ"]) and f["AD"] == [int(x) for x in s["AD"].split(",")] and f["NL"] == int(s["NL"]), (where, f, line)
    assert abs(f["PB"] - float(s["PB"])) <= 5e-5 + 1e-9, (where, "PB", f["PB"], s["PB"])
    if debug and "AD0" in s:
        for k in (0, 1):
            assert str(f[f"AD{k}"]) == s[f"AD{k}"] and str(f[f"DP{k}"]) == s[f"DP{k}"], (where, k, f, line)


# ---- seeded pools ---------------------------------------------------------------------------------------------------------------------
def _variant(rng, position, ref, alt, depth, vf, gt=None, nl=20):
    support = int(round(depth * vf))
    t = R.set_type(ref, alt)
    if t == "Reference":
        support = int(round(depth * (1 - rng.random() * 0.01)))
        genotype = gt or "HomozygousRef"
        refsup = support
    else:
        refsup = max(0, depth - support - int(rng.integers(0, 3)))
        genotype = gt or ("HomozygousAlt" if vf > 0.9 else "HeterozygousAltRef")
    cov = [depth // 2, depth - depth // 2, 0]
    sup = [support // 2, support - support // 2, 0]
    return {"position": int(position), "ref": ref, "alt": alt, "type": t, "genotype": genotype, "total_coverage": int(depth), "allele_support": support,
            "reference_support": refsup, "variant_qscore": int(rng.choice([0, 17, 30, 75, 100])), "genotype_qscore": int(rng.integers(0, 101)), "noise_level": int(nl),
            "filters": int(rng.choice([0, 0, 0, 1 << 4, 1 << 5, (1 << 0) | (1 << 3)])), "sb": float(rng.choice([1e-10, 0.0, 0.31, 2.5e-5])),
            "num_no_calls": int(rng.integers(0, 5)), "coverage_by_dir": cov, "support_by_dir": sup, "bias_bits": int(rng.integers(0, 8))}


ALTS = (("A", "T"), ("A", "G"), ("A", "C"), ("A", "ATG"), ("ACC", "A"), ("AC", "TT"), ("AC", "A"), ("A", "AT"))
VFS = (0.0005, 0.004, 0.009, 0.0105, 0.02, 0.029, 0.031, 0.08, 0.45, 0.97)
DEFENSIVE = ("AltAndNoCall", "HemizygousAlt", "RefAndNoCall", "HemizygousRef", "HemizygousNoCall")


def make_pools(rng, n_positions, start=1000):
    """two pools of one chromosome: every kind of position SelectPairs and GetComparisonCase tell apart, frequencies around both thresholds,
    depths around MinimumCoverage, unequal noise levels, the genotypes DoDefensiveGenotyping rewrites"""
    pool_a, pool_b = [], []
    position = int(start)
    for _ in range(n_positions):
        position += int(rng.choice([1, 1, 1, 2, 40]))
        kind = int(rng.integers(14))
        depth = lambda: int(rng.choice([0, 4, 9, 10, 300, 5000, 30000]))
        nl = lambda: int(rng.choice([20, 20, 20, 35, 2, 12]))
        vf = lambda: float(rng.choice(VFS))
        alts = [ALTS[i] for i in rng.permutation(len(ALTS))[:3]]
        ref_gt = lambda: str(rng.choice(["HomozygousRef", "HomozygousRef", "RefLikeNoCall", "RefAndNoCall", "HemizygousRef", "HemizygousNoCall"]))
        alt_gt = lambda: (str(rng.choice(["AltAndNoCall", "HemizygousAlt", "AltLikeNoCall", "HomozygousAlt"])) if rng.random() < 0.25 else None)
        ref = lambda: _variant(rng, position, "A", ".", depth(), 0, ref_gt(), nl())
        alt = lambda k: _variant(rng, position, alts[k][0], alts[k][1], max(depth(), 1), vf(), alt_gt(), nl())
        if kind == 0:                       # ref + ref
            pool_a.append(ref()); pool_b.append(ref())
        elif kind == 1:                     # alt + the same alt
            pool_a.append(alt(0)); pool_b.append(alt(0))
        elif kind == 2:                     # ref + alt, alt + ref
            first, second = (pool_a, pool_b) if rng.random() < 0.5 else (pool_b, pool_a)
            first.append(ref()); second.append(alt(0))
        elif kind == 3:                     # one pool only
            (pool_a if rng.random() < 0.5 else pool_b).append(ref() if rng.random() < 0.5 else alt(0))
        elif kind == 4:                     # ref + {alt, alt', alt''}
            pool_a.append(ref()); pool_b.extend(alt(k) for k in range(int(rng.integers(2, 4))))
        elif kind == 5:                     # {alt, alt', alt''} + ref
            pool_b.append(ref()); pool_a.extend(alt(k) for k in range(int(rng.integers(2, 4))))
        elif kind == 6:                     # alt sets that agree in part
            pool_a.extend([alt(0), alt(1)]); pool_b.extend([alt(1), alt(2)])
        elif kind == 7:                     # different alternates
            pool_a.append(alt(0)); pool_b.append(alt(1))
        elif kind == 8:                     # {ref, alt} + {ref, alt'}: the references agree, the alternates stand alone
            pool_a.extend([ref(), alt(0)]); pool_b.extend([ref(), alt(1)])
        elif kind == 9:                     # ref + low alternates that all come out as references: two or more consensus references
            pool_a.append(_variant(rng, position, "A", ".", 5000, 0, "HomozygousRef", nl()))
            pool_b.extend(_variant(rng, position, alts[k][0], alts[k][1], 5000, 0.004, None, nl()) for k in range(3))
        elif kind == 10:                    # a deletion against a reference
            pool_a.append(_variant(rng, position, "ACC", "A", 3000, vf(), None, nl())); pool_b.append(ref())
        elif kind == 11:                    # the same alternate, one pool almost without it: pool bias
            pool_a.append(_variant(rng, position, "A", "T", 4000, 0.2, None, 20)); pool_b.append(_variant(rng, position, "A", "T", 4000, float(rng.choice([0.0, 0.001, 0.19])), None, 20))
        elif kind == 12:                    # every genotype DoDefensiveGenotyping rewrites
            gt = DEFENSIVE[int(rng.integers(len(DEFENSIVE)))]
            is_alt = gt in ("AltAndNoCall", "HemizygousAlt")
            pool_a.append(_variant(rng, position, "A", "T" if is_alt else ".", 500, 0.3, gt, nl())); pool_b.append(ref() if rng.random() < 0.5 else alt(0))
        else:                               # low depth on both sides
            pool_a.append(_variant(rng, position, "A", ".", int(rng.integers(0, 6)), 0, "HomozygousRef", nl()))
            pool_b.append(_variant(rng, position, "A", ".", int(rng.integers(0, 5)), 0, "HomozygousRef", nl()))
    return pool_a, pool_b
