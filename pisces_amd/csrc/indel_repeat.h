// indel_repeat.h — FilterType.IndelRepeatLength (-RepeatFilter_ToBeRetired, FILTER R<n>): the repeat length of ONE allele in the reference
// around it (AlleleProcessor.ComputeIndelRepeatLength, src/exe/Pisces/Logic/VariantCalling/AlleleProcessor.cs:80-107, with
// CheckVariantRepeatCount :109-135, SimplifyRepeatUnit :140-155 and GetRepeatLength :160-213), one source for the host and the device, as
// exact_span.h and amplicon_bias.h are for their decisions.
//   indel_repeat.cpp             the host form: pisces_hip_indel_repeat_length
//   indel_repeat_kernels.hip.h   the device form: indel_repeat_kernel over the records of call_spanning_kernel
// The reference cuts two strings out of the chromosome (50 bases upstream of stringPos = position - 1, 50 from it on, each clamped to the
// sequence, :86-103), joins them again (:130) and scans the joined string.  The two pieces are neighbours in the chromosome, so the joined
// string is one stretch of it: nothing is copied here, `bases[i]` is ref[first + i].  The repeat unit is a length: the variant bases'
// shortest period, and `repeatUnit[index]` is the variant bases' own byte.  GetRepeatLength's quirks are kept as written (the early 1, the
// backtrack that only runs while currentPos > 0, the count that stops one unit and one base short of the stretch's end).
#pragma once
#include <stdint.h>

#include "../../include/pisces_hip.h"

#if defined(__HIPCC__)
#define PISCES_RHD __host__ __device__
#else
#define PISCES_RHD
#endif

namespace pisces {
namespace indel_repeat {

constexpr int32_t kFlankingBaseCount = 50;   // AlleleProcessor.FlankingBaseCount (:14)
constexpr int32_t kSubstringThrows = -1;     // String.Substring's ArgumentOutOfRangeException (:100, :102): a position decidedly outside the chromosome

// referenceBases...ToUpper() (:100-103): the handle's chromosome is upper-cased already, a host's own array need not be
PISCES_RHD inline uint8_t upper(uint8_t b) { return (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b; }

// SimplifyRepeatUnit (:140-155): the prefix grows by one base until Split by it leaves only empty pieces, (pieces - 1) * prefix length ==
// length, i.e. until the bases are whole copies of the prefix; a prefix of every length below n is tried, the bases themselves never are.
PISCES_RHD inline int32_t simplified_unit_length(const uint8_t* v, int32_t n)
{
    for (int32_t p = 1; p < n; p++) {
        if (n % p != 0) continue;
        bool copies = true;
        for (int32_t j = p; j < n && copies; j++) copies = v[j] == v[j - p];
        if (copies) return p;
    }
    return n;
}

// The repeat length of (category, position, alleles) over ref[0, ref_length), ref[i] = position i + 1; kSubstringThrows where the reference throws.
PISCES_RHD inline int32_t length(int32_t category, int32_t position, const uint8_t* ref_allele, int32_t ref_len, const uint8_t* alt_allele,
                                 int32_t alt_len, const uint8_t* ref, int64_t ref_length)
{
    if (ref_length <= 0) return 0;   // :82
    if (category != PISCES_CAT_INSERTION && category != PISCES_CAT_DELETION && category != PISCES_CAT_SNV) return 0;   // :83
    // GetFlankingBases (:86-103): upstream [upstreamBegin, stringPos - 1], downstream [stringPos, stringPos + 49], both clamped
    const int64_t string_pos = (int64_t)position - 1;
    // downstream: Substring(max(0, stringPos), ...) of length min(stringPos + 49, L - 1) - max(0, stringPos) + 1, negative beyond either end;
    // the upstream Substring only throws further out (stringPos > L + 50)
    if (string_pos > ref_length || string_pos < -(int64_t)kFlankingBaseCount) return kSubstringThrows;
    const int64_t first = string_pos > kFlankingBaseCount ? string_pos - kFlankingBaseCount : 0;        // bases[0]
    const int64_t upstream = (string_pos > 0 ? string_pos : 0) - first;                                  // upstreamFlankingBases.Length
    const int64_t end = string_pos + kFlankingBaseCount < ref_length ? string_pos + kFlankingBaseCount : ref_length;
    const int32_t n_bases = (int32_t)(end - first);                                                      // bases.Length, <= 100
    // CheckVariantRepeatCount (:111-127): an SNV has no variant bases -> GetRepeatLength's "nonsense input" 0 (:163)
    const uint8_t* v;
    int32_t v_len;
    if (category == PISCES_CAT_INSERTION) { v = alt_allele + 1; v_len = alt_len - 1; }        // AlternateAllele.Substring(1)
    else if (category == PISCES_CAT_DELETION) { v = ref_allele + 1; v_len = ref_len - 1; }    // ReferenceAllele.Substring(1)
    else return 0;
    if (v_len <= 0) return 0;
    int32_t cur = (int32_t)upstream + 1;
    const int32_t unit = simplified_unit_length(v, v_len);
    const uint8_t* bases = ref + first;
    // GetRepeatLength (:160-213)
    const int32_t last = n_bases - unit - 1;
    if (cur + unit + 1 > n_bases) return 1;   // "a deletion is larger than the number of downstream flanking bases" — and every indel two bases from the end
    auto match = [&](int32_t at) {
        for (int32_t k = 0; k < unit; k++)
            if (upper(bases[at + k]) != v[k]) return false;
        return true;
    };
    int32_t previous = cur;
    while (cur > 0) {   // backtrack
        if (!match(cur)) break;
        previous = cur;
        cur -= unit;
    }
    cur = previous;
    int32_t repeats = 0;
    while (cur <= last) {
        if (!match(cur)) break;
        cur += unit;
        repeats++;
    }
    return repeats;
}

}  // namespace indel_repeat
}  // namespace pisces
