// indel_repeat.cpp — the host form of indel_repeat.h: pisces_hip_indel_repeat_length, for a caller that filters its own alleles.
// Pure host code, no device, no handle.
#include "indel_repeat.h"

extern "C" {

int32_t pisces_hip_indel_repeat_length(int32_t category, int32_t position, const uint8_t* ref_allele, int32_t ref_len, const uint8_t* alt_allele,
                                       int32_t alt_len, const uint8_t* ref_bases, int64_t ref_length)
{
    if (ref_length < 0 || ref_len < 0 || alt_len < 0 || (ref_length > 0 && !ref_bases)) return PISCES_E_INVALID_ARG;
    // the allele whose bases are read must be there, anchor base included (AlternateAllele.Substring(1) / ReferenceAllele.Substring(1) throw on "")
    if (category == PISCES_CAT_INSERTION && (alt_len < 1 || !alt_allele)) return PISCES_E_INVALID_ARG;
    if (category == PISCES_CAT_DELETION && (ref_len < 1 || !ref_allele)) return PISCES_E_INVALID_ARG;
    const int32_t n = pisces::indel_repeat::length(category, position, ref_allele, ref_len, alt_allele, alt_len, ref_bases, ref_length);
    return n == pisces::indel_repeat::kSubstringThrows ? PISCES_E_INVALID_ARG : n;
}

}  // extern "C"
