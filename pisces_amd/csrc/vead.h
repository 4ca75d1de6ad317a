// vead.h — Scylla's read pass (src/lib/VariantPhasing): what ONE read says about the variant sites of a neighbourhood ("vead"), and which
// reads a neighbourhood looks at.  One source for the host and the device, as exact_span.h, venn.h and vqr.h are for their stages.
//   surface_vead.inc.h     the host forms: pisces_hip_vead_site_states, pisces_hip_vead_neighborhood_info, pisces_hip_vead_groups
//   vead_kernels.hip.h     the device form: vead_states_kernel compiles the same source
// Restated without building strings:
//   next_segment    VeadFinder.SetCandidateVariantsFoundInRead (VeadFinder.cs:348-457): the read's CIGAR as match / insertion / deletion
//                   segments.  The walk starts at referencePosition = Position - 1 (Position 1-based here) and cycle index 0; a segment
//                   stands at referencePosition + 1, an insertion or deletion one base before that.  S advances the cycle index, M both
//                   counters, I the cycle index, D the reference position.  EVERY OTHER OPERATION (N, =, X, H, P) ADVANCES NOTHING and
//                   leaves no segment: the reference's switch has no case for them.  Reproduced, not repaired.
//   site_state      VeadFinder.MatchReadVariantsWithVcfVariants (:86-249) for one site, with CheckVariantSequenceForMatchInVariantSiteFromRead
//                   (:263-302) and HaveWeSeenEvidenceForAReferenceCall (:41-72).  What the code does, not what its comments say: when the
//                   loop has "gone past" the site, the result it assigns there is overwritten by the IDontKnow / switch tail below the
//                   loop, so the last state the loop computed decides.
//   bounds, clipped VcfNeighborhood.SetRangeOfInterest (VcfNeighborhood.cs:82-132) and NeighborhoodReadFilter, over the sites in the
//                   caller's order (nothing is sorted here: List.Sort is not stable, the caller passes VcfVariantSites as they are).
// Two spans of a read are in play and both are kept: the walk above ends at Position + (M + D lengths) (lastPosInAlignment); the filter's
// EndPosition is Position + GetReferenceSpan() - 1, which counts M D N = X (BamCommon.cs:119).
//
// The group key.  The reference groups veads by the string Vead.ToVariantSequence(); two state vectors print the same exactly when they are
// equal, with one exception: a site whose own alleles are one equal base (A>A) prints "A>A" for PISCES_VEAD_REF and for PISCES_VEAD_ALT.
// site_state gives PISCES_VEAD_REF for that case.  For the same reason a REF whose first reference base is the letter N or X (it prints
// "N>N" / "X>X") is given as PISCES_VEAD_NONE / PISCES_VEAD_OTHER.  So equal strings are equal states everywhere.
//
// Where the reference would index past the read (a CIGAR longer than the read, a zero-length insertion at the read's end) a base reads as
// 'N' and a quality as failing: the library's batches have passed Read.ValidateCigar, these lines only keep a malformed one inside its arrays.
#pragma once
#include <stdint.h>

#include "../../include/pisces_hip.h"

#if defined(__HIPCC__)
#define PISCES_HD __host__ __device__
#else
#define PISCES_HD
#endif

namespace pisces {
namespace vead {

// VeadFinder.StateOfPhasingSiteInRead
enum State : int32_t { kFoundThis = 0, kInsufficient = 1, kDifferent = 2, kReference = 3, kIDontKnow = 4 };

struct ReadView {
    int32_t position;   // Read.Position, 1-based
    const uint8_t* op;
    const uint32_t* len;
    int32_t n_cigar;
    const uint8_t* bases;
    const uint8_t* quals;
    int64_t n_bases;
};

struct Segment {
    uint8_t type;       // 'M', 'I', 'D'
    bool no_data;       // VariantSite.HasNoData: an insertion / deletion that failed the base-call quality
    uint32_t length;
    int64_t position;   // VcfReferencePosition
    int64_t cycle;      // overallCycleIndex at the segment's first base (deletion: the base behind it)
};
struct Cursor {
    int32_t c = 0;
    int64_t ref_pos = 0, cycle = 0;
};

PISCES_HD inline int32_t qual_at(const ReadView& r, int64_t c) { return (c >= 0 && c < r.n_bases) ? (int32_t)r.quals[c] : -1000000; }
// the match segment's allele: the read's base, 'N' below the minimum quality (:384-391)
PISCES_HD inline uint8_t masked_base(const ReadView& r, int64_t c, int32_t min_q)
{
    if (c < 0 || c >= r.n_bases) return 'N';
    return (int32_t)r.quals[c] < min_q ? (uint8_t)'N' : r.bases[c];
}

PISCES_HD inline Cursor begin(const ReadView& r)
{
    Cursor k;
    k.c = 0;
    k.ref_pos = (int64_t)r.position - 1;
    k.cycle = 0;
    return k;
}

// the next segment of the read, false behind the last
PISCES_HD inline bool next_segment(const ReadView& r, int32_t min_q, Cursor& k, Segment& s)
{
    while (k.c < r.n_cigar) {
        const uint8_t t = r.op[k.c];
        const uint32_t L = r.len[k.c];
        k.c++;
        const int64_t vs = k.ref_pos + 1;
        if (t == 'S') {
            k.cycle += L;
        } else if (t == 'M') {
            s.type = 'M'; s.no_data = false; s.length = L; s.position = vs; s.cycle = k.cycle;
            k.cycle += L;
            k.ref_pos += L;
            return true;
        } else if (t == 'I') {   // the FIRST inserted base's quality decides (:404)
            s.type = 'I'; s.no_data = qual_at(r, k.cycle) < min_q; s.length = L; s.position = vs - 1; s.cycle = k.cycle;
            k.cycle += L;
            return true;
        } else if (t == 'D') {   // the bases on both sides, by the reference's index rule (:426-435)
            const int32_t after = k.cycle < r.n_bases ? qual_at(r, k.cycle) : qual_at(r, k.cycle - 1);
            const int32_t before = k.cycle > 0 ? qual_at(r, k.cycle - 1) : after;
            s.type = 'D'; s.no_data = !(before >= min_q && after >= min_q); s.length = L; s.position = vs - 1; s.cycle = k.cycle;
            k.ref_pos += L;
            return true;
        }
    }
    return false;
}

// lastPosInAlignment (:455)
PISCES_HD inline int64_t last_position(const ReadView& r)
{
    int64_t p = r.position;
    for (int32_t c = 0; c < r.n_cigar; c++)
        if (r.op[c] == 'M' || r.op[c] == 'D') p += r.len[c];
    return p;
}
// Read.EndPosition = Position + CigarData.GetReferenceSpan() - 1
PISCES_HD inline int64_t end_position(int32_t position, const uint8_t* op, const uint32_t* len, int32_t n_cigar)
{
    int64_t span = 0;
    for (int32_t c = 0; c < n_cigar; c++)
        if (op[c] == 'M' || op[c] == 'D' || op[c] == 'N' || op[c] == '=' || op[c] == 'X') span += len[c];
    return (int64_t)position + span - 1;
}

// CheckVariantSequenceForMatchInVariantSiteFromRead for a match segment: outside -> insufficient, equal to alt -> this variant, an N ->
// insufficient, equal to the site's reference allele bytes -> reference, else different
PISCES_HD inline State check_match(const ReadView& r, int32_t min_q, const Segment& s, int64_t site_pos, const uint8_t* ref, int32_t ref_len,
                                   const uint8_t* alt, int32_t alt_len)
{
    const int64_t idx = site_pos - s.position;
    if (idx + alt_len > (int64_t)s.length || idx < 0) return kInsufficient;
    bool eq_alt = true, has_n = false, eq_ref = ref_len == alt_len;
    for (int32_t k = 0; k < alt_len; k++) {
        const uint8_t b = masked_base(r, s.cycle + idx + k, min_q);
        eq_alt = eq_alt && b == alt[k];
        has_n = has_n || b == 'N';
        if (eq_ref) eq_ref = b == ref[k];
    }
    if (eq_alt) return kFoundThis;
    if (has_n) return kInsufficient;
    if (eq_ref) return kReference;
    return kDifferent;
}

// HaveWeSeenEvidenceForAReferenceCall: a one-base ref[0] > ref[0] site at the site's position against every match segment
PISCES_HD inline bool reference_evidence(const ReadView& r, int32_t min_q, int64_t site_pos, uint8_t ref0)
{
    Cursor k = begin(r);
    Segment s;
    while (next_segment(r, min_q, k, s)) {
        if (s.type != 'M') continue;
        const State st = check_match(r, min_q, s, site_pos, &ref0, 1, &ref0, 1);
        if (st == kFoundThis || st == kReference) return true;
    }
    return false;
}

// One site of MatchReadVariantsWithVcfVariants' loop.  `last` = last_position(r).  *in_range: the site counts into numSitesFoundInRead.
PISCES_HD inline uint8_t site_state(const ReadView& r, int32_t min_q, int64_t last, const PiscesVeadSite& site, const uint8_t* alleles, bool* in_range)
{
    const uint8_t* const ref = alleles + site.allele_offset;
    const uint8_t* const alt = ref + site.ref_len;
    const int64_t true_first = (int64_t)site.position + (site.ref_len != site.alt_len ? 1 : 0);   // VariantSite.TrueFirstBaseOfDiff
    *in_range = !(true_first < (int64_t)r.position || true_first > last);
    if (!*in_range) return PISCES_VEAD_NONE;
    const uint8_t type = site.ref_len > site.alt_len ? 'D' : site.ref_len < site.alt_len ? 'I' : 'M';   // GetVariantType
    const bool same_base = site.ref_len == 1 && site.alt_len == 1 && ref[0] == alt[0];

    State result = kIDontKnow;
    Cursor k = begin(r);
    Segment s;
    while (next_segment(r, min_q, k, s)) {
        if (s.type != type) continue;
        if (result == kFoundThis) break;
        if ((int64_t)site.position < s.position) break;   // gone past: what is assigned there is overwritten below
        if (type == 'M') {
            result = check_match(r, min_q, s, site.position, ref, site.ref_len, alt, site.alt_len);
        } else if (s.position == (int64_t)site.position) {
            if (s.no_data) {
                result = kInsufficient;
            } else if (type == 'I') {   // the inserted bases as they are against alt[1:]
                bool eq = (int64_t)s.length == (int64_t)site.alt_len - 1;
                for (uint32_t b = 0; eq && b < s.length; b++) eq = (s.cycle + b < r.n_bases) && r.bases[s.cycle + b] == alt[1 + b];
                result = eq ? kFoundThis : kDifferent;
            } else {                    // the deleted lengths
                result = (int64_t)site.ref_len - site.alt_len == (int64_t)s.length ? kFoundThis : kDifferent;
            }
        }
    }
    // no segment of the type at all (:109-120) and the IDontKnow tail (:203-210) come to the same: reference when a match segment says so
    if (result == kIDontKnow && reference_evidence(r, min_q, site.position, ref[0])) result = kReference;
    uint8_t state = PISCES_VEAD_NONE;
    if (result == kFoundThis) state = same_base ? PISCES_VEAD_REF : PISCES_VEAD_ALT;
    else if (result == kDifferent) state = PISCES_VEAD_OTHER;
    else if (result == kReference) state = PISCES_VEAD_REF;
    // (a site that is itself N>N or X>X prints its REF like NONE or OTHER)
    if (state == PISCES_VEAD_REF && ref[0] == 'N') state = PISCES_VEAD_NONE;
    if (state == PISCES_VEAD_REF && ref[0] == 'X') state = PISCES_VEAD_OTHER;
    return state;
}

// FindVariantResults for one read: a state a site, the number of sites in range (the read is a vead when that reaches
// min_number_variants_in_read, :248)
PISCES_HD inline int32_t read_states(const ReadView& r, int32_t min_q, const PiscesVeadSite* sites, int32_t n_sites, const uint8_t* alleles, uint8_t* states)
{
    const int64_t last = last_position(r);
    int32_t found = 0;
    for (int32_t i = 0; i < n_sites; i++) {
        bool in_range;
        states[i] = site_state(r, min_q, last, sites[i], alleles, &in_range);
        found += in_range ? 1 : 0;
    }
    return found;
}

// ---- the neighbourhood's side -----------------------------------------------------------------------------------------------------
struct Bounds { int32_t first, last_with_look_ahead, soft_clip_end_before, soft_clip_pos_after; };

PISCES_HD inline Bounds bounds(const PiscesVeadSite* sites, int32_t begin, int32_t end)
{
    Bounds b;
    const PiscesVeadSite& f = sites[begin];
    const PiscesVeadSite& l = sites[end - 1];
    b.first = f.position;
    b.last_with_look_ahead = f.position;
    for (int32_t i = begin; i < end; i++) {
        const int32_t look = sites[i].position + (sites[i].alt_len > sites[i].ref_len ? sites[i].alt_len : sites[i].ref_len);
        if (look > b.last_with_look_ahead) b.last_with_look_ahead = look;
    }
    b.soft_clip_end_before = f.ref_len != f.alt_len ? f.position : f.position - 1;
    b.soft_clip_pos_after = l.position + l.ref_len;
    return b;
}

// NeighborhoodReadFilter.IsClippedWithinNeighborhood
PISCES_HD inline bool clipped(int32_t position, int64_t end, bool starts_s, bool ends_s, const Bounds& b)
{
    if (starts_s && position >= b.soft_clip_end_before && position <= b.soft_clip_pos_after) return true;
    return ends_s && end >= b.soft_clip_end_before && end <= b.soft_clip_pos_after;
}

// One read of VeadGroupSource.GetVeadGroups' loop (:56-75): the clip test FIRST, whether or not the read is used afterwards, then
// ShouldSkipRead (EndPosition < FirstPositionOfInterest), then PastNeighborhood (the scan stops there)
enum Verdict : int32_t { kSkip = 0, kUse = 1, kPast = 2 };
PISCES_HD inline Verdict scan_read(int32_t position, int64_t end, bool starts_s, bool ends_s, const Bounds& b, bool* is_clipped)
{
    *is_clipped = clipped(position, end, starts_s, ends_s, b);
    if (end < b.first) return kSkip;
    if (position > b.last_with_look_ahead) return kPast;
    return kUse;
}

// the 2-bit packing of a vead's states: site i in bits 2 * (i % 32) of word i / 32
PISCES_HD inline int32_t key_words(int32_t n_sites) { return (n_sites + 31) / 32; }

}  // namespace vead
}  // namespace pisces
