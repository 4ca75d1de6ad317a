"""AlleleProcessor.ComputeIndelRepeatLength in plain Python — TEST INFRASTRUCTURE, the statement the library's
pisces_hip_indel_repeat_length and indel_repeat_kernel are held to (tests/test_indel_repeat_cpu.py, tests/test_indel_repeat_gpu.py).

Written from src/exe/Pisces/Logic/VariantCalling/AlleleProcessor.cs:80-213 with Python strings, statement by statement as the C# reads:
the two flanks are cut out and joined again, the repeat unit is a string, String.Split is str.split.  It shares no code with the library
(csrc/indel_repeat.h indexes the chromosome and keeps the unit as a length).
"""
FLANKING_BASE_COUNT = 50   # :14


class ArgumentOutOfRange(Exception):
    """String.Substring's ArgumentOutOfRangeException."""


def substring(s, start, length=None):
    """String.Substring(startIndex[, length]): throws where Python's slice would quietly clamp."""
    if length is None:
        length = len(s) - start
    if start < 0 or length < 0 or start > len(s) or start + length > len(s):
        raise ArgumentOutOfRange((start, length, len(s)))
    return s[start:start + length]


def flanking_bases(position, reference):
    """:86-103 (upstream, downstream)"""
    string_pos = position - 1
    upstream_begin = string_pos - FLANKING_BASE_COUNT
    upstream_end = string_pos - 1
    downstream_begin = string_pos
    downstream_end = string_pos + FLANKING_BASE_COUNT - 1
    if upstream_begin < 0:
        upstream_begin = 0
    if downstream_begin < 0:
        downstream_begin = 0
    if downstream_end >= len(reference):
        downstream_end = len(reference) - 1
    if upstream_end >= len(reference):
        upstream_end = len(reference) - 1
    upstream = ""
    if upstream_end >= 0:
        upstream = substring(reference, upstream_begin, upstream_end - upstream_begin + 1).upper()
    downstream = substring(reference, downstream_begin, downstream_end - downstream_begin + 1).upper()
    return upstream, downstream


def simplify_repeat_unit(repeat_unit):
    """:140-155"""
    if len(repeat_unit) == 0:
        return ""
    sb = repeat_unit[0:1]
    for i in range(1, len(repeat_unit)):
        test_for_repeats = repeat_unit.split(sb)
        is_valid_repeat_unit = len(repeat_unit) == (len(test_for_repeats) - 1) * len(sb)
        if is_valid_repeat_unit:
            break
        sb += repeat_unit[i]
    return sb


def get_repeat_length(bases, current_pos, repeat_unit, trace=None):
    """:160-213.  trace (a dict) receives which way the call went: 'early' (the return 1 of :168), 'backtracked' (the number of units the
    backtrack loop stepped over, the one at the start included), 'cut' (the forward count ended at lastPosition with the unit still matching
    where there was room to look)."""
    num_repeat_bases = len(repeat_unit)
    if num_repeat_bases == 0:
        return 0
    last_position = len(bases) - num_repeat_bases - 1
    required_length = current_pos + num_repeat_bases + 1
    if required_length > len(bases):
        if trace is not None:
            trace["early"] = True
        return 1
    previous_pos = current_pos
    steps = 0
    while current_pos > 0:
        if bases[current_pos:current_pos + num_repeat_bases] != repeat_unit:
            break
        previous_pos = current_pos
        current_pos -= num_repeat_bases
        steps += 1
    current_pos = previous_pos
    repeat_length = 0
    while current_pos <= last_position:
        if bases[current_pos:current_pos + num_repeat_bases] != repeat_unit:
            break
        current_pos += num_repeat_bases
        repeat_length += 1
    if trace is not None:
        trace["backtracked"] = steps
        trace["cut"] = current_pos > last_position and repeat_length > 0 and bases[current_pos:current_pos + num_repeat_bases] == repeat_unit
    return repeat_length


def indel_repeat_length(category, position, ref_allele, alt_allele, reference, trace=None):
    """ComputeIndelRepeatLength :80-107 + CheckVariantRepeatCount :109-135.  category: "Snv" / "Mnv" / "Insertion" / "Deletion" /
    "Reference"."""
    if not reference:
        return 0
    if category not in ("Insertion", "Deletion", "Snv"):
        return 0
    upstream, downstream = flanking_bases(position, reference)
    current_position = 0
    if upstream:
        current_position = len(upstream)
    variant_bases = ""
    if category == "Insertion":
        variant_bases = substring(alt_allele, 1)
        current_position += 1
    if category == "Deletion":
        variant_bases = substring(ref_allele, 1)
        current_position += 1
    bases = "%s%s" % (upstream, downstream)
    repeat_unit = simplify_repeat_unit(variant_bases)
    return get_repeat_length(bases, current_position, repeat_unit, trace)


def is_flagged(threshold, category, position, ref_allele, alt_allele, reference):
    """ApplyFilters :39, :52-57: never on a Reference allele, only with a threshold above 0."""
    if category == "Reference" or threshold is None or not threshold > 0:
        return False
    return threshold <= indel_repeat_length(category, position, ref_allele, alt_allele, reference)
