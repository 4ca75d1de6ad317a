#!/usr/bin/env python3
"""Extracts the known-answer table of the reference's RMxN filter test into tests/golden/rmxn_cases.json.

Reads  <reference>/src/test/Pisces.Calculators.Tests/UnitTests/RMxNFilterCalculatorTests.cs  as DATA: every ExecuteRMxNMnvTest /
ExecuteRMxNIndelTest call of RMxN() (:22-86) becomes one case (source line, variant bases, the sequence with its '*', the expected
repeat count, the unit-length limit, and the alleles the harness :91-125 builds of it: an MNV call one SNV or MNV, an indel call one
insertion and one deletion); the two calls that stand in comments ("SCYLLA") are named as not part of the table; the six assertions
of the harness (:137-165) become `assertions` (the repetitions as an offset from the expected count, the frequency limit, the answer).
Nothing of the test code is stored.  Run from the repo root in the build container (the reference is not available on the GPU box):
    python tests/golden/extract_rmxn_cases.py /root/reference
"""
import json
import os
import re
import sys

ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
rel = "Pisces.Calculators.Tests/UnitTests/RMxNFilterCalculatorTests.cs"
lines = open(os.path.join(ref_root, "src/test", rel), encoding="utf-8-sig").read().splitlines()

CALL = re.compile(r'ExecuteRMxN(Mnv|Indel|)Test\(\s*"([A-Z]+)"\s*,\s*"([A-Z*]+)"\s*,\s*(\d+)\s*(?:,\s*(\d+|AlleleCategory\.\w+)\s*)?\)')


def alleles_of(kind, variant, sequence):
    """ExecuteRMxNTest :103-125."""
    coordinate = sequence.index("*")
    clean = sequence.replace("*", "")
    anchor = clean[coordinate - 1]
    if kind == "Mnv":
        category = "Mnv" if len(variant) > 1 else "Snv"
        return [{"category": category, "position": coordinate, "ref": clean[coordinate - 1:coordinate - 1 + len(variant)], "alt": variant}]
    return [{"category": "Insertion", "position": coordinate, "ref": anchor, "alt": anchor + variant},
            {"category": "Deletion", "position": coordinate, "ref": anchor + variant, "alt": anchor}]   # (whether or not the sequence holds them)


cases, not_in_table = [], []
for no, text in enumerate(lines, 1):
    m = CALL.search(text)
    if not m or "private void" in text:
        continue
    kind, variant, sequence, repeats, limit = m.groups()
    if "//" in text[:m.start()]:
        not_in_table.append({"line": no, "variant": variant, "sequence": sequence, "repeats": int(repeats), "why": "the call stands in a comment"})
        continue
    assert kind in ("Mnv", "Indel"), (no, text)
    cases.append({"line": no, "kind": kind, "variant": variant, "sequence": sequence, "repeats": int(repeats),
                  "max_unit": int(limit) if limit else len(variant), "alleles": alleles_of(kind, variant, sequence)})

# the harness: the allele's counts and what it asserts under which settings
frequency = coverage = None
assertions, setting = [], {}
in_harness = False
for no, text in enumerate(lines, 1):
    code = text.split("//")[0]
    m = re.search(r"double\s+variantFrequncy\s*=\s*([0-9.]+)", code)
    if m:
        frequency = float(m.group(1))
    if "private void ExecuteRMxNTest(" in code:
        in_harness = True
    if not in_harness:
        continue
    m = re.search(r"TotalCoverage\s*=\s*(\d+)", code)
    if m:
        coverage = int(m.group(1))
    m = re.search(r"RMxNFilterFrequencyLimit\s*=\s*([0-9.]+)f", code)
    if m:
        setting["frequency_limit"] = float(m.group(1))
    m = re.search(r"RMxNFilterMinRepetitions\s*=\s*expectedRepeatLength\s*(?:([+-])\s*(\d+))?\s*;", code)
    if m:
        setting["min_rep_delta"] = int((m.group(1) or "+") + (m.group(2) or "0"))
    m = re.search(r"Assert\.(True|False)\(RMxNCalculator\.ShouldFilter\(", code)
    if m:
        assertions.append({"line": no, "min_rep_delta": setting["min_rep_delta"], "frequency_limit": setting["frequency_limit"],
                           "flagged": 1 if m.group(1) == "True" else 0})

assert len(cases) == 36 and sum(len(c["alleles"]) for c in cases) == 55 and len(not_in_table) == 2 and len(assertions) == 6, \
    (len(cases), len(not_in_table), len(assertions))
assert frequency == 0.20 and coverage == 1000
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rmxn_cases.json")
json.dump({"_source": rel + ": RMxN :22-86 (every ExecuteRMxNMnvTest / ExecuteRMxNIndelTest call), the alleles of ExecuteRMxNTest :103-125 "
                      "(position = the 1-based position of the base before '*'; a deletion's reference allele is anchor + variant bases whether or not the "
                      "sequence holds them), the allele's counts :134-135 and the six assertions :137-165 (min_rep_delta: RMxNFilterMinRepetitions minus the "
                      "expected repeat count; 'not flagged at N + 1' is asserted twice); max_unit: RMxNFilterMaxLengthRepeat (default: the variant's length)",
           "frequency": frequency, "total_coverage": coverage, "allele_support": int(coverage * frequency),
           "assertions": assertions, "not_in_table": not_in_table, "cases": cases}, open(out, "w"), indent=0)
print(out, len(cases), "cases,", sum(len(c["alleles"]) for c in cases), "alleles,", len(assertions), "assertions")
