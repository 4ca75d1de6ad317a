"""Extracts every ExecuteTest(...) call of the reference's ExactCoverageCalculatorTests.cs (Insertion, Deletion, MNV) as data:

    python tests/golden/extract_exact_cases.py <path to ExactCoverageCalculatorTests.cs> > tests/golden/exact_coverage_cases.json

The three facts build one ReadCoverageSummary after another with object initialisers and then change single properties between calls, so the
script replays those statements in file order: `new ReadCoverageSummary { ... }`, `readSummary.X = ...;` and `ExecuteTest(category, expected,
readSummary)`.  A case is what the summary holds when ExecuteTest is reached.  ExecuteTest puts every allele at position 10 with four
inserted / deleted / changed bases (its variantPosition default and its allele strings).  The script fails unless it extracted as many
cases as the file has ExecuteTest call sites.
"""
import json
import re
import sys

PROPERTY = r"(ClipAdjustedStartPosition|ClipAdjustedEndPosition|CigarString|Cigar|DirectionString)"
VALUE = r"(?:new CigarAlignment\(\"([^\"]*)\"\)|\"([^\"]*)\"|(-?\d+))"


def extract(text):
    body = text[:text.index("private void ExecuteTest")]
    call_sites = len(re.findall(r"\bExecuteTest\s*\(", body))
    position = int(re.search(r"int variantPosition = (\d+)", text).group(1))
    lengths = {"Insertion": len(re.search(r'case AlleleCategory\.Insertion:.*?AlternateAllele = "(\w+)"', text, re.S).group(1)) - 1,
               "Deletion": len(re.search(r'case AlleleCategory\.Deletion:.*?ReferenceAllele = "(\w+)"', text, re.S).group(1)) - 1,
               "Mnv": len(re.search(r'default:.*?AlternateAllele = "(\w+)"', text, re.S).group(1))}
    statement = re.compile(r"(new ReadCoverageSummary)|readSummary\." + PROPERTY + r"\s*=\s*" + VALUE + r"\s*;|(?<![\w.])" + PROPERTY + r"\s*=\s*" + VALUE + r"\s*[,}\n]"
                           r"|ExecuteTest\(AlleleCategory\.(\w+),\s*(null|DirectionType\.(\w+)),\s*readSummary\)")
    cases, summary = [], {}
    for m in statement.finditer(body):
        if m.group(1):
            summary = {}
        elif m.group(2) or m.group(6):
            name = m.group(2) or m.group(6)
            cigar, string, number = (m.group(3), m.group(4), m.group(5)) if m.group(2) else (m.group(7), m.group(8), m.group(9))
            key = {"ClipAdjustedStartPosition": "cs", "ClipAdjustedEndPosition": "ce", "CigarString": "cigar", "Cigar": "cigar", "DirectionString": "directions"}[name]
            summary[key] = int(number) if number is not None else (cigar if cigar is not None else string)
        else:
            assert set(summary) == {"cs", "ce", "cigar", "directions"}, summary
            category = m.group(10)
            cases.append({"category": category.lower(), "position": position, "length": lengths[category], "cs": summary["cs"], "ce": summary["ce"],
                          "cigar": summary["cigar"], "directions": summary["directions"], "expected": None if m.group(11) == "null" else m.group(12).lower()})
    assert len(cases) == call_sites, f"{len(cases)} cases extracted, {call_sites} ExecuteTest call sites in the file"
    return cases


if __name__ == "__main__":
    with open(sys.argv[1], encoding="utf-8-sig") as fp:
        cases = extract(fp.read())
    print(json.dumps({"source": "src/test/Pisces.Calculators.Tests/UnitTests/ExactCoverageCalculatorTests.cs", "n_cases": len(cases), "cases": cases}, indent=1))
