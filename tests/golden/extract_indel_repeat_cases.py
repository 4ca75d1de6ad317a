#!/usr/bin/env python3
"""Extracts the data of the reference's two indel-repeat tests into tests/golden/indel_repeat_cases.json.

Reads  <reference>/src/test/Pisces.Tests/UnitTests/VariantCalling/VariantProcessorTests.cs  as DATA: every ExecuteRepeatTest call of
IndelRepeat() (:82-127) becomes one row (source line, variantBases, repeatUnit, repeatsInReference, threshold, flagged), and the facts
of IndelRepeat_ChromosomeEdgeCases() (:129-189) are read off its statements: the chromosome (75 x "A"), the allele (insertion A>AA),
the threshold (the eighth argument of AlleleProcessor.Process), the loop's range of flagged positions, the two positions that are not
flagged and the one where Process throws.  How ExecuteRepeatTest expands a row (:343-420) is stated in tests/test_indel_repeat_cpu.py;
nothing of the test code is stored.  Run from the repo root where the reference's sources are available:
    python tests/golden/extract_indel_repeat_cases.py <root of the reference's checkout>
"""
import json
import os
import re
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
ref_root = sys.argv[1]
rel = "Pisces.Tests/UnitTests/VariantCalling/VariantProcessorTests.cs"
lines = open(os.path.join(ref_root, "src/test", rel), encoding="utf-8-sig").read().splitlines()

CALL = re.compile(r'^\s*ExecuteRepeatTest\(\s*"([A-Z]+)"\s*,\s*"([A-Z]+)"\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(true|false)\s*\)\s*;')
rows = []
for no, text in enumerate(lines, 1):
    m = CALL.match(text)
    if m:
        rows.append({"line": no, "variant_bases": m.group(1), "repeat_unit": m.group(2), "repeats_in_reference": int(m.group(3)),
                     "threshold": int(m.group(4)), "flagged": m.group(5) == "true"})

# the edge-case test
start = next(i for i, t in enumerate(lines) if "public void IndelRepeat_ChromosomeEdgeCases()" in t)
end = next(i for i in range(start, len(lines)) if "public void RMxN()" in lines[i])
body = "\n".join(t.split("//")[0] for t in lines[start:end])
m = re.search(r'Enumerable\.Repeat\("([A-Z])",\s*(\d+)\)', body)
base, length = m.group(1), int(m.group(2))
assert re.search(r"for \(int i = 0; i < chrReference\.Sequence\.Length - 1; i\+\+\)", body)
alleles = set(re.findall(r'ReferenceAllele = "([A-Z]+)";\s*\w+\.AlternateAllele = "([A-Z]+)";', body))
assert alleles == {("A", "AA")} and len(set(re.findall(r"\.Type = AlleleCategory\.(\w+);", body))) == 1
thresholds = set(re.findall(r"AlleleProcessor\.Process\(\w+, 0\.01f, 0, 0,\s*true, 0, 0, (\d+), null", body))
assert thresholds == {"2"}, thresholds
assert "variantAtLastPosition.ReferencePosition = chrReference.Sequence.Length;" in body
assert "variantAtSecondToLastPosition.ReferencePosition = chrReference.Sequence.Length - 1;" in body
assert "variantOutsideOfChromosome.ReferencePosition = chrReference.Sequence.Length + 2;" in body
assert "Assert.Throws<ArgumentOutOfRangeException>" in body
edge = {"sequence_base": base, "sequence_length": length, "category": "Insertion", "ref": "A", "alt": "AA", "threshold": 2,
        "flagged_positions": [0, length - 2], "not_flagged_positions": [length - 1, length], "throws_positions": [length + 2]}

assert rows and all(r["line"] in range(82, 128) for r in rows), len(rows)
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "indel_repeat_cases.json")
json.dump({"_source": rel + ": IndelRepeat :82-127 (every ExecuteRepeatTest call) and IndelRepeat_ChromosomeEdgeCases :129-189 (flagged_positions: "
                      "the inclusive range of ReferencePosition values the loop :139-153 asserts the filter for; the variant's ReferencePosition is "
                      "used as it stands, 0 included)",
           "rows": rows, "edge": edge}, open(out, "w"), indent=0)
print(out, len(rows), "rows")
