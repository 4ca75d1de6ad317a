"""Writes tests/golden/vqr_cases.json from the reference's VariantQualityRecalibration test data (README_vqr.md has the sources).

    python tests/golden/extract_vqr_cases.py <reference root>

Data only: the rows of four VCFs and two expected .recal files as numbers and strings, the numbers of six counts files, the suspect
list, the options the reference's tests set, the buffers of EdgeIssueCountDataTests.DidWeDetectAnEdge as the test leaves them before each
assertion, and the facts RecalTests asserts.  Body lines are picked by field count (two of the files carry a byte-order mark, one of
them encoded twice, in front of a header line)."""
import json
import os
import sys

DATA = "src/test/VariantQualityRecalibration.Tests/TestData"
VCFS = ["TestWithArtifacts.vcf", "ExpectedDirty.vcf.recal", "TestEdgeExample.vcf", "ExpectedEdgeExample.vcf.recal", "TestSignatureSorter.vcf",
        "FindEdges.vcf"]
COUNTS = ["Dirty.counts", "Expected.counts", "ExpectedGivenLociNum.counts", "Expected.edgecounts", "ExpectedGivenLociNum.edgecounts"]
CATEGORIES = ["AtoC", "AtoG", "AtoT", "CtoA", "CtoG", "CtoT", "GtoA", "GtoC", "GtoT", "TtoA", "TtoC", "TtoG", "Insertion", "Deletion", "Reference",
              "Other"]


def vcf_rows(path):
    rows = []
    for raw in open(path, "rb").read().decode("utf-8", errors="replace").splitlines():
        f = raw.split("\t")
        if len(f) < 10 or f[0].lstrip("\ufeff").startswith("#"):
            continue
        info = dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv)
        sample = dict(zip(f[8].split(":"), f[9].split(":")))
        rows.append({"chrom": f[0], "pos": int(f[1]), "ref": f[3], "alt": f[4], "qual": int(float(f[5])), "filter": f[6],
                     "dp": int(info["DP"]), "ad": [int(x) for x in sample["AD"].split(",")], "gq": int(sample["GQ"]), "nl": int(sample["NL"])})
    return rows


def counts_file(path):
    by, n = {}, None
    for line in open(path, "rb").read().decode("utf-8", errors="replace").splitlines():
        f = line.split()
        if len(f) == 2 and f[0] in CATEGORIES:
            by[f[0]] = int(float(f[1]))
        elif len(f) == 2 and f[0] == "AllPossibleVariants":
            n = int(float(f[1]))
    assert sorted(by) == sorted(CATEGORIES) and n is not None, path
    return {"by_category": [by[c] for c in CATEGORIES], "num_possible_variants": n}


def did_we_detect_an_edge():
    """EdgeIssueCountDataTests.cs:14-102 replayed: seven alleles of chr1 at 10..16, coverage 100; every assertion with the buffer as it is then.
    A slot is [chromosome, position, coverage] or null."""
    buf = [["chr1", 10 + i, 100] for i in range(7)]
    out = []

    def check(expected, line):
        out.append({"line": line, "test_index": 3, "buffer": [None if b is None else list(b) for b in buf], "expected": expected})

    check(False, 24)
    buf[2][2] = 2; check(True, 30)
    buf[3][2] = 400; check(True, 34); buf[3][2] = 100
    buf[2][2] = 400; check(False, 41)
    buf[2][2] = 100; buf[2][0] = "chrM"; check(True, 46); buf[2][0] = "chr1"
    buf[0][1] = buf[1][1] = buf[2][1] = 12; check(False, 53)
    buf[3][2] = 400; check(True, 57)
    buf[3][1] = buf[4][1] = buf[5][1] = buf[6][1] = 12; check(True, 64)
    buf[3][2] = 100; check(False, 68)
    buf[4][1] = buf[5][1] = buf[6][1] = 14; check(True, 74)
    buf[4][1], buf[5][1], buf[6][1] = 13, 14, 15; buf[0][2] = 10; check(True, 82)
    buf[0][2] = 100; buf[6][2] = 10; check(True, 87)
    buf[6][2] = 100; buf[3][2] = 400; check(True, 92); buf[3][2] = 100
    buf[6] = None; check(True, 97)
    buf[6] = buf[2]; buf[3] = None; check(False, 102)
    return out


def main(root):
    data = os.path.join(root, DATA)
    cases = {
        "categories": CATEGORIES,
        "vcfs": {name: vcf_rows(os.path.join(data, name)) for name in VCFS},
        "counts": {name: counts_file(os.path.join(data, name)) for name in COUNTS},
        "edgevariants": [[f[0].lstrip("\ufeff"), int(f[1]), f[3], f[4]] for f in
                         (ln.split("\t") for ln in open(os.path.join(data, "Expected.edgevariants"), encoding="utf-8").read().splitlines() if ln.strip())],
        "options": {
            # RecalTests.cs:28-40 (the counts come from Dirty.counts, not from the VCF)
            "RecalibrateDirtyVcf": {"z_factor": 0, "max_qscore": 66, "filter_qscore": 0, "base_q_noise": 30, "do_basic_checks": 1,
                                    "do_amplicon_position_checks": 0},
            # EdgeIssueRecalTests.cs:25-27 (Program.Main: every other option at its default)
            "RecalibrateDirtyVcfs": {"do_basic_checks": 1, "do_amplicon_position_checks": 1, "extent_of_edge_region": 2,
                                     "alignment_warning_threshold": 1},
            # SignatureSorter_FFPETests.cs / SignatureSorter_AlignmentIssueTests.cs:35-43, 63-71
            "WriteCountsFile": {"loci_count": -1}, "WriteCountsFileGivenLociCounts": {"loci_count": 1000},
            "WriteEdgeCountsFile": {"loci_count": -1, "do_basic_checks": 0, "do_amplicon_position_checks": 1, "extent_of_edge_region": 2},
            "WriteEdgeCountsFileGivenLociCounts": {"loci_count": 1000, "do_basic_checks": 0, "do_amplicon_position_checks": 1, "extent_of_edge_region": 2},
        },
        "did_we_detect_an_edge": did_we_detect_an_edge(),
        # RecalTests.UpdateVariant / InsertNewQ / HaveInfoToUpdateQ (RecalTests.cs:103-213)
        "update_variant": {
            "allele": {"total_coverage": 100, "reference_support": 90, "allele_support": 10, "genotype_qscore": 72, "noise_level": 20, "variant_qscore": 666},
            "category": "CtoA", "rate": 12, "max_qscore": 100,
            "expected": {"variant_qscore": 10, "genotype_qscore": 10, "noise_level": 12},
            # (filter_qscore, filters before, filters after), :113-146 (the third case adds OffTarget to what the second left)
            "filter_cases": [[5, [], []], [30, [], ["LowVariantQscore"]], [30, ["LowVariantQscore", "OffTarget"], ["LowVariantQscore", "OffTarget"]],
                             [30, ["LowVariantQscore"], ["LowVariantQscore"]], [30, ["LowVariantQscore", "OffTarget"], ["LowVariantQscore", "OffTarget"]]],
            "insert_new_q": {"new_q": 42, "expected": {"variant_qscore": 42, "genotype_qscore": 42, "noise_level": 12}},
            "have_info": {"depth": 100, "call_count": 10},
        },
    }
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vqr_cases.json")
    with open(out, "w") as fp:
        json.dump(cases, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(out, {k: len(v) for k, v in cases["vcfs"].items()})


if __name__ == "__main__":
    main(sys.argv[1])
