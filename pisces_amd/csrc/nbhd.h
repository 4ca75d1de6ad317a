// nbhd.h — Scylla's neighbourhoods of phasable variants (src/lib/VariantPhasing): which called rows of ONE chromosome chain into a
// neighbourhood, which neighbourhoods are kept, and the order their sites are handed to the read pass in.  One source for the host and the
// device, as vead.h and venn.h are for their stages.
//   surface_nbhd.inc.h     the host form pisces_hip_nbhd_build and the launches of pisces_hip_nbhd_build_device
//   nbhd_kernels.hip.h     the device form: every kernel decides through the functions below
// Restated without lists or strings:
//   forced_report   NeighborhoodBuilder.GetBatchOfCallableNeighborhoods (NeighborhoodBuilder.cs:74):
//                       if (currentAllele.Filters.Contains(FilterType.ForcedReport)) continue;
//                   before anything else: such a row is neither eligible nor the "last variant site" of the proximity test.
//   eligible        NeighborhoodBuilder.IsEligibleVariant (:147-181):
//                       if ((allele.IsRefType) || (allele.IsNocall)) return false;
//                       if (allele.Type == AlleleCategory.Unsupported) ... return false;
//                       if (_phasableVariantCriteria.HetVariantsOnly) if (genotype == Genotype.HomozygousAlt) return false;
//                       if (!_phasableVariantCriteria.PassingVariantsOnly) return true;
//                       return (filters.Count() == 0);
//                   CalledAllele.IsNocall is Alt12LikeNoCall, AltLikeNoCall, HemizygousNoCall, RefLikeNoCall; RefAndNoCall and AltAndNoCall are
//                   NOT no-calls there.  ChrToProcessArray stays with the host: a call is one chromosome.
//   passing         VariantSite.IsAcceptablePhasingCandidate (VariantSite.cs:77-83): filters.Count == 0, whatever PassingVariantsOnly says.
//                   A "filter" is one of bits 0..13 of filter_bits; bits 14..15 are the phase-set index (PISCES_FILTERBITS_PHASE).
//   proximal        NeighborhoodBuilder.IsProximal (:184-187):
//                       Math.Abs(variantSite1.VcfReferencePosition - otherSite.VcfReferencePosition) < phasingDistance
//                   taken against _lastVariantSite, which line :97 sets to every ELIGIBLE row, chained or not (the `continue` of :85 skips
//                   it for the others).  The first eligible row has no predecessor: `new VariantSite()` has a null ReferenceName.
//   chaining        FitVariantsInNeighborhood (:190-235): a proximal pair starts a neighbourhood of (last, current) unless the last
//                   neighbourhood ends at last's position (LastPositionIsNotMatch), then current is appended.  On rows that ascend and a
//                   distance of at least 1 that is: the maximal runs of two or more consecutive eligible rows, each proximal to the one
//                   before it.  (If the last neighbourhood ends at last's position, last is in it: were it not, the row of that
//                   neighbourhood at the same position would be its eligible predecessor at distance 0, and it would have been appended.)
//                   _maxNumNbhdsInBatch and the "hanging" neighbourhood (:212-225, :238-246) decide only WHICH call returns a
//                   neighbourhood; tests/nbhd_ref.py keeps them and shows that they drop out.
//   dropped         ConvertToCallableNeighborhoods (:129):
//                       if (nbhd.PassingVariants < _phasableVariantCriteria.MinPassingVariantsInNbhd && nbhd.NonPassingVariants > 0) continue;
//                   A dropped neighbourhood was counted by rawNumNeighborhoods (:101) and took a number (AddNewNeighborhoodToBatch :251-253).
//   site order      VcfNeighborhood.OrderVariantSitesByFirstTrueStartPosition (VcfNeighborhood.cs:70-78), called by CallableNeighborhood's
//                   constructor (CallableNeighborhood.cs:98), sorts by VariantSite.TrueFirstBaseOfDiff (VariantSite.cs:18-21):
//                       IsInsertionOrDeletion() ? VcfReferencePosition + 1 : VcfReferencePosition          (ref length != alt length)
//                   and then writes OriginalAlleleFromVcf back in the PRE-sort order:
//                       var indexes = VcfVariantSites.Select(vs => vs.OriginalAlleleFromVcf).ToList();  VcfVariantSites.Sort();
//                       for (...) VcfVariantSites[i].OriginalAlleleFromVcf = indexes[i];
//                   Kept: site s holds the alleles of row site_row[s] and the original allele of row site_original[s].
//                   The sort is taken as STABLE (List.Sort is an insertion sort up to 16 elements and unspecified among equal keys above
//                   that: a stated deviation).  On rows that ascend a stable sort by that key moves nothing across positions: the rows of a
//                   position p have keys p (equal lengths) and p + 1 (indels); everything in front of them has a key of at most p and
//                   comes first among equals, everything behind a key of at least p + 1 and comes last among equals.  So within one
//                   position the equal-length alleles go in front of the indels, each kind in input order, and that is all (sorted_slot).
//   bounds          VcfNeighborhood.SetRangeOfInterest over the sorted sites: vead.h's bounds(), not restated; LastPositionOfInterestInVcf
//                   (the last sorted site's position, :85) is added by the callers.
//   reference       CallableNeighborhood.cs:102-107: Substring(FirstPositionOfInterest - 1, LastPositionOfInterestWithLookAhead -
//                   FirstPositionOfInterest) of the chromosome, or that many 'R' without one (reference_byte).
#pragma once
#include <stdint.h>

#include "../../include/pisces_hip.h"
#include "vead.h"

namespace pisces {
namespace nbhd {

// what a row is to the builder
enum RowBits : uint8_t { kForced = 1, kEligible = 2, kPassing = 4, kNoAlleles = 8 };
// an eligible row among its neighbours
enum LinkBits : uint8_t { kMember = 1, kHead = 2, kTail = 4, kIsPassing = 8 };

constexpr uint32_t kFilterMask = 0x3FFFu;   // bits 14..15 of filter_bits are the phase-set index

struct View {   // PiscesVennRows less its count
    const PiscesCalledAllele* recs;
    const int32_t* cand_index;
    const PiscesCandidate* cands;
    const uint8_t* alleles;
};

PISCES_HD inline bool is_nocall(uint32_t genotype)   // CalledAllele.IsNocall
{
    return genotype == PISCES_GT_ALT12_LIKE_NOCALL || genotype == PISCES_GT_ALT_LIKE_NOCALL || genotype == PISCES_GT_HEMI_NOCALL ||
           genotype == PISCES_GT_REF_LIKE_NOCALL;
}
PISCES_HD inline bool forced_report(uint32_t filter_bits) { return (filter_bits >> PISCES_FILTER_FORCED_REPORT) & 1u; }
PISCES_HD inline bool passing(uint32_t filter_bits) { return (filter_bits & kFilterMask) == 0; }

PISCES_HD inline bool eligible(const PiscesNbhdCriteria& c, uint32_t info, uint32_t filter_bits)
{
    const uint32_t category = PISCES_INFO_CATEGORY(info), genotype = PISCES_INFO_GENOTYPE(info);
    if (category == PISCES_CAT_REFERENCE || is_nocall(genotype)) return false;
    if (category > PISCES_CAT_REFERENCE) return false;   // AlleleCategory.Unsupported
    if (c.het_variants_only && genotype == PISCES_GT_HOM_ALT) return false;
    if (!c.passing_variants_only) return true;
    return passing(filter_bits);
}

// the row against the last ELIGIBLE row; rows ascend, so the difference is Math.Abs of itself
PISCES_HD inline bool proximal(int32_t position, int32_t last_position, int32_t phasing_distance)
{
    return (int64_t)position - (int64_t)last_position < (int64_t)phasing_distance;
}

PISCES_HD inline bool dropped(int64_t n_passing, int64_t n_non_passing, int32_t min_passing_variants_in_nbhd)
{
    return n_passing < (int64_t)min_passing_variants_in_nbhd && n_non_passing > 0;
}

PISCES_HD inline bool has_candidate(const View& v, int64_t r) { return v.cand_index && v.cand_index[r] >= 0; }

// the lengths of a row's alleles (VCF form, anchor base included); false: a row that needs a candidate's bytes and has none
PISCES_HD inline bool allele_lengths(const View& v, int64_t r, int32_t* ref_len, int32_t* alt_len)
{
    if (has_candidate(v, r)) {
        const PiscesCandidate& c = v.cands[v.cand_index[r]];
        *ref_len = c.ref_len;
        *alt_len = c.alt_len;
        return c.ref_len >= 1 && c.alt_len >= 1;   // (an empty allele is no allele in VCF form)
    }
    *ref_len = *alt_len = 1;
    const uint32_t category = PISCES_INFO_CATEGORY(v.recs[r].info);
    return !(category == PISCES_CAT_INSERTION || category == PISCES_CAT_DELETION || category == PISCES_CAT_MNV);
}

PISCES_HD inline uint8_t base_of_code(uint32_t code)
{
    return code == PISCES_ALLELE_A ? 'A' : code == PISCES_ALLELE_G ? 'G' : code == PISCES_ALLELE_C ? 'C' : code == PISCES_ALLELE_T ? 'T' : 'N';
}

// ref bytes then alt bytes of row r to dst
PISCES_HD inline void copy_alleles(const View& v, int64_t r, uint8_t* dst)
{
    if (has_candidate(v, r)) {
        const PiscesCandidate& c = v.cands[v.cand_index[r]];
        const uint8_t* const src = v.alleles + c.allele_offset;
        for (int32_t k = 0; k < c.ref_len + c.alt_len; k++) dst[k] = src[k];
        return;
    }
    dst[0] = base_of_code(PISCES_INFO_REF(v.recs[r].info));
    dst[1] = base_of_code(PISCES_INFO_ALT(v.recs[r].info));
}

// RowBits of row r
PISCES_HD inline uint8_t row_bits(const View& v, const PiscesNbhdCriteria& c, int64_t r)
{
    const uint32_t info = v.recs[r].info, filter_bits = v.recs[r].filter_bits;
    int32_t ref_len, alt_len;
    uint8_t bits = allele_lengths(v, r, &ref_len, &alt_len) ? 0 : kNoAlleles;
    if (passing(filter_bits)) bits |= kPassing;
    if (forced_report(filter_bits)) return bits | kForced;
    if (eligible(c, info, filter_bits)) bits |= kEligible;
    return bits;
}

// the position the proximity test of eligible row e > 0 is taken against: that of the last ELIGIBLE row, e - 1, whatever lies between
PISCES_HD inline int32_t last_site_position(const View& v, const int32_t* e_row, int64_t e) { return v.recs[e_row[e - 1]].position; }

// LinkBits of eligible row e of n_eligible (e_row: the rows of the eligible rows)
PISCES_HD inline uint8_t link_bits(const View& v, const int32_t* e_row, int64_t n_eligible, int64_t e, int32_t phasing_distance)
{
    const bool to_last = e > 0 && proximal(v.recs[e_row[e]].position, last_site_position(v, e_row, e), phasing_distance);
    const bool to_next = e + 1 < n_eligible && proximal(v.recs[e_row[e + 1]].position, last_site_position(v, e_row, e + 1), phasing_distance);
    uint8_t bits = 0;
    if (to_last || to_next) bits |= kMember;
    if (to_next && !to_last) bits |= kHead;
    if (to_last && !to_next) bits |= kTail;
    return bits;
}

// Where the stable sort by TrueFirstBaseOfDiff puts eligible row e of the neighbourhood [first, end) (indices among the eligible rows,
// which ascend by position): *group is the first row of e's position, the result the index e lands at, *bytes_in_front the allele bytes
// of the rows of that position sorted in front of it.
PISCES_HD inline int64_t sorted_slot(const int32_t* position, const int32_t* ref_len, const int32_t* alt_len, int64_t first, int64_t end, int64_t e,
                                     int64_t* group, int64_t* bytes_in_front)
{
    int64_t g0 = e, g1 = e + 1;
    while (g0 > first && position[g0 - 1] == position[e]) g0--;
    while (g1 < end && position[g1] == position[e]) g1++;
    const bool indel = ref_len[e] != alt_len[e];
    int64_t in_front = 0, bytes = 0;
    for (int64_t i = g0; i < g1; i++) {
        if (i == e) continue;
        const bool other_indel = ref_len[i] != alt_len[i];
        const bool front = other_indel == indel ? i < e : indel;   // equal lengths go in front of indels, each kind in input order
        if (front) { in_front++; bytes += (int64_t)ref_len[i] + alt_len[i]; }
    }
    *group = g0;
    *bytes_in_front = bytes;
    return g0 + in_front;
}

// NbhdReferenceSequenceSubstring's length and its byte k
PISCES_HD inline int64_t reference_length(const vead::Bounds& b) { return (int64_t)b.last_with_look_ahead - b.first; }
PISCES_HD inline uint8_t reference_byte(const uint8_t* reference, int64_t reference_len, const vead::Bounds& b, int64_t k)
{
    const int64_t from = (int64_t)b.first - 1;
    const bool inside = reference && from >= 0 && from + reference_length(b) <= reference_len;
    return inside ? reference[from + k] : (uint8_t)'R';
}

// one kept neighbourhood's info from its sorted sites
PISCES_HD inline PiscesNbhdInfo make_info(const PiscesVeadSite* sites, int32_t begin, int32_t end, int32_t raw_index, int32_t n_passing, int32_t n_non_passing,
                                          int64_t ref_offset)
{
    const vead::Bounds b = vead::bounds(sites, begin, end);
    PiscesNbhdInfo o;
    o.raw_index = raw_index;
    o.n_passing = n_passing;
    o.n_non_passing = n_non_passing;
    o.first = b.first;
    o.last_in_vcf = sites[end - 1].position;
    o.last_with_look_ahead = b.last_with_look_ahead;
    o.soft_clip_end_before = b.soft_clip_end_before;
    o.soft_clip_pos_after = b.soft_clip_pos_after;
    o.ref_len = (int32_t)reference_length(b);
    o.reserved = 0;
    o.ref_offset = ref_offset;
    return o;
}

}  // namespace nbhd
}  // namespace pisces
