"""RMxNCalculator (lib/Pisces.Calculators/RMxNCalculator.cs:19-133) over Python strings — TEST INFRASTRUCTURE, no tests in here.

The plain statement every other form of the filter is held to: the oracle's (oracle/pisces_oracle.c), the device's two SNV forms
(device_math.hip.h) and its spanning form (kernels.hip.h).  Written from the C# line by line, no arithmetic of its own: substrings,
loops and one float32 quotient.
"""
import numpy as np

SNV, MNV, INSERTION, DELETION = "Snv", "Mnv", "Insertion", "Deletion"


def _compare_substring(str1, str2, start_pos2):
    """VcfVariantUtilities.CompareSubstring (Pisces.IO/VcfVariantUtilities.cs:547-558): str1 stands in str2 at start_pos2.  Like the C#, an
    index beyond str2 raises: no valid allele gets there (the callers guard both directions)."""
    assert start_pos2 >= 0
    for i in range(len(str1)):
        if str1[i] != str2[start_pos2 + i]:
            return False
    return True


def length_for_indel(variant_position, variant_bases, reference_bases, max_repeat_unit_length):
    """ComputeRMxNLengthForIndel :49-95.  variant_position: the string index the ratchet starts from (the 1-based position of the base
    before the inserted / deleted bases)."""
    max_repeats_found = 0
    prefixes, suffixes = [], []
    length = len(variant_bases)
    for i in range(length - min(max_repeat_unit_length, length), length):
        prefixes.append(variant_bases[0:length - i])
        suffixes.append(variant_bases[i:i + length - i])
    for bookend in prefixes + suffixes:
        back_peek_position = variant_position
        while True:   # keep ratcheting backward as long as this motif is repeating
            new_back_peek_position = back_peek_position - len(bookend)
            if new_back_peek_position < 0:
                break
            if not _compare_substring(bookend, reference_bases, new_back_peek_position):
                break
            back_peek_position = new_back_peek_position
        repeat_count = 0
        current_position = back_peek_position
        while True:   # read forward from the first instance of the motif
            if current_position + len(bookend) > len(reference_bases):
                break
            if not _compare_substring(bookend, reference_bases, current_position):
                break
            repeat_count += 1
            current_position += len(bookend)
        if repeat_count > max_repeats_found:
            max_repeats_found = repeat_count
    return max_repeats_found


INT_MAX = 2147483647


def component_lengths(category, position, ref, alt, chromosome, max_unit):
    """ComputeComponentRMxNLengths :104-133."""
    component2 = INT_MAX
    if category == INSERTION:
        component1 = length_for_indel(position, alt[1:], chromosome, max_unit)
    elif category == DELETION:
        component1 = length_for_indel(position, ref[1:], chromosome, max_unit)
    else:
        assert category in (SNV, MNV), category
        component1 = length_for_indel(position - 1, ref, chromosome, max_unit)
        insertion1 = length_for_indel(position + len(ref) - 1, alt, chromosome, max_unit)
        insertion2 = length_for_indel(position - 1, alt, chromosome, max_unit)
        component2 = max(insertion1, insertion2)
    return component1, component2


def frequency(support, coverage):
    """CalledAllele.Frequency: a float32 quotient, capped at 1; 0 without coverage."""
    if coverage == 0:
        return np.float32(0)
    return min(np.float32(support) / np.float32(coverage), np.float32(1))


def should_filter(category, position, ref, alt, chromosome, max_unit, min_rep, limit, support, coverage):
    """ShouldFilter :19-38.  max_unit None (or < 0, the library's form of it): no settings, never flagged.  limit: the float32
    RMxNFilterFrequencyLimit."""
    if max_unit is None or max_unit < 0:
        return False
    if frequency(support, coverage) >= np.float32(limit):   # high frequency alleles escape
        return False
    c1, c2 = component_lengths(category, position, ref, alt, chromosome, max_unit)
    return min(c1, c2) >= min_rep
