// exact_span.h — CoverageMethod.Exact (-coveragemethod exact): which direction ONE read counts in for ONE spanning allele
// (ExactCoverageCalculator.CalculateSpanning, src/lib/Pisces.Calculators/ExactCoverageCalculator.cs:62-96, with GetIndexBoundaries :162-199
// and GetDirection :114-153), one source for the host and the device, as amplicon_bias.h is for the amplicon-bias decision.
//   exact_span.cpp         the host form: pisces_hip_exact_span_direction
//   exact_kernels.hip.h    the device form: exact_span_kernel over the read store's summaries
// What a read leaves behind (Read.GetCoverageSummary, Read.cs:613-622): its clip-adjusted start CS = Position - leading soft clip and end
// CE = EndPosition + trailing soft clip (GetPrefixClip / GetSuffixClip skip H and stop at the first other operation, BamCommon.cs:787-824),
// its CIGAR and the run-length form of its per-base directions.  The allele asks with a span [preceding, trailing]
// (ExactCoverageCalculator.cs:18-42: deletion p .. p + Length + 1, MNV p - 1 .. p + Length, insertion p .. p + 1).
//
// The position map of a read with more than one direction run is built from CS - GetPrefixClip() (:90): Position less TWICE the leading
// soft clip, handed to a function that gives the first aligned base the position it was handed (Read.UpdatePositionMap, Read.cs:564-592).
// Reproduced as written; so are the -2 marks of soft-clipped bases and the two soft-clip special cases of GetIndexBoundaries.  Nothing
// here builds the two maps: a read's bases are walked operation by operation, twice at the most.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PISCES_HD __host__ __device__
#else
#define PISCES_HD
#endif

namespace pisces {
namespace exact {

constexpr int32_t kDropped = -1;        // the read does not span the allele: it counts nowhere
constexpr int32_t kNoIndices = -2;      // GetDirection's InvalidDataException: neither a base at or before `preceding` nor one at or behind `trailing`
constexpr int32_t kMalformed = -3;      // (host form only) the direction runs are longer than the CIGAR's read span
constexpr int32_t kStitched = 2;        // DirectionType: Forward 0, Reverse 1, Stitched 2

PISCES_HD inline bool op_ref_span(uint8_t t) { return t == 'M' || t == 'D' || t == 'N' || t == '=' || t == 'X'; }   // CigarExtensions.cs:356-369
PISCES_HD inline bool op_read_span(uint8_t t) { return t == 'M' || t == 'I' || t == 'S' || t == '=' || t == 'X'; }  // :370-383

// CigarAlignment.GetPrefixClip / GetSuffixClip
PISCES_HD inline int64_t prefix_clip(const uint8_t* op, const uint32_t* len, int32_t n)
{
    int64_t clip = 0;
    for (int32_t c = 0; c < n; c++) {
        if (op[c] == 'S') clip += len[c];
        else if (op[c] != 'H') break;
    }
    return clip;
}
PISCES_HD inline int64_t suffix_clip(const uint8_t* op, const uint32_t* len, int32_t n)
{
    int64_t clip = 0;
    for (int32_t c = n - 1; c >= 0; c--) {
        if (op[c] == 'S') clip += len[c];
        else if (op[c] != 'H') break;
    }
    return clip;
}
PISCES_HD inline int64_t read_span(const uint8_t* op, const uint32_t* len, int32_t n)
{
    int64_t s = 0;
    for (int32_t c = 0; c < n; c++)
        if (op_read_span(op[c])) s += len[c];
    return s;
}
PISCES_HD inline int64_t ref_span(const uint8_t* op, const uint32_t* len, int32_t n)
{
    int64_t s = 0;
    for (int32_t c = 0; c < n; c++)
        if (op_ref_span(op[c])) s += len[c];
    return s;
}

// The tests that need no walk (:68-70).  first_is_i / last_is_i: the STRICT first / last operation is an insertion
// (HasOperationAtOpIndex(0, 'I') / (0, 'I', fromEnd), CigarExtensions.cs:38-44): 5M3I2S does not end in one.
PISCES_HD inline bool spans(int64_t cs, int64_t ce, bool first_is_i, bool last_is_i, int64_t preceding, int64_t trailing)
{
    if (ce < preceding || cs > trailing) return false;
    if (ce == preceding && !last_is_i) return false;
    if (cs == trailing && !first_is_i) return false;
    return true;
}

// GetIndexBoundaries + GetDirection for a read with more than one direction run.  dir_at(i): DirectionType of the read's base i,
// 0 <= i < read span.  Returns 0 / 1 / 2 or kNoIndices.
template <typename DirAt>
PISCES_HD inline int32_t walk_direction(int64_t cs, const uint8_t* op, const uint32_t* len, int32_t n_cigar, DirAt dir_at, int64_t preceding, int64_t trailing)
{
    const int64_t map_start = cs - prefix_clip(op, len, n_cigar);   // (:90: the clip comes off a second time)
    // ---- GetIndexBoundaries: the last base at a position in [0, preceding], the first base at a position >= trailing
    int64_t start_index = -1, end_index = -1, n = 0;
    int64_t first_mark = 0, last_mark = 0;   // positionMap[0] / positionMap[Length - 1]
    {
        int64_t p = map_start;
        for (int32_t c = 0; c < n_cigar; c++) {
            const uint8_t t = op[c];
            const int64_t l = len[c];
            const bool rd = op_read_span(t), rf = op_ref_span(t);
            if (rd && l > 0) {
                const int64_t mark = t == 'S' ? -2 : -1;
                if (n == 0) first_mark = rf ? p : mark;
                last_mark = rf ? p + l - 1 : mark;
                if (rf) {
                    // positions p .. p + l - 1 at indices n .. n + l - 1
                    const int64_t lo = p > 0 ? p : 0, hi = preceding < p + l - 1 ? preceding : p + l - 1;   // positionAtIndex >= 0 && <= startPosition
                    if (hi >= lo) start_index = n + (hi - p);
                    if (end_index < 0 && p + l - 1 >= trailing) end_index = n + (trailing > p ? trailing - p : 0);
                } else if (end_index < 0 && mark >= trailing) {
                    end_index = n;   // (a mark is -1 or -2: only a span that ends below 0 sees it as "at or behind")
                }
                n += l;
            }
            if (rf) p += l;
        }
    }
    // a read that ends in a soft clip, e.g. 5M5D5S: the first soft-clipped base behind the start index (:177-186)
    const bool special_end = start_index >= 0 && end_index < 0 && n > 0 && last_mark == -2;
    // ... and one that starts in one: the last soft-clipped base in front of the end index (:188-196)
    const bool special_start = end_index >= 0 && start_index < 0 && n > 0 && first_mark == -2;
    if (special_end || special_start) {
        int64_t i = 0, p = map_start;
        for (int32_t c = 0; c < n_cigar; c++) {
            const uint8_t t = op[c];
            const int64_t l = len[c];
            const bool rd = op_read_span(t), rf = op_ref_span(t);
            if (rd && l > 0) {
                // the indices [a, b] of this operation that hold -2: a soft clip's, or — a read whose shifted map starts below 0 — the one
                // aligned base that lies at position -2 (the reference compares the map's entries with -2, whatever put them there)
                int64_t a = 0, b = -1;
                if (t == 'S') { a = i; b = i + l - 1; }
                else if (rf && p <= -2 && p + l - 1 >= -2) { a = b = i + (-2 - p); }
                if (b >= a) {
                    if (special_end && end_index < 0 && b > start_index) end_index = a > start_index ? a : start_index + 1;
                    if (special_start && a < end_index) start_index = b < end_index - 1 ? b : end_index - 1;
                }
                i += l;
            }
            if (rf) p += l;
        }
    }
    // ---- GetDirection
    if (start_index == -1 && end_index == -1) return kNoIndices;
    int32_t direction = 0;
    if (end_index == start_index + 1) {   // the indices are right next to each other
        if (start_index == -1) direction = dir_at(end_index);
        else {
            direction = dir_at(start_index);
            if (direction == kStitched) direction = dir_at(end_index);
        }
    } else {
        const int64_t stop = end_index == -1 ? n : end_index;   // go to the end of the read
        for (int64_t i = start_index + 1; i <= stop - 1; i++) {
            direction = dir_at(i);
            if (direction == kStitched) break;
        }
    }
    return direction;
}

// The whole per-read decision from a summary whose directions are runs (the reference's DirectionInfo): kDropped, 0 / 1 / 2, kNoIndices,
// or kMalformed when the runs are longer than the CIGAR's read span (Read.UpdateDirectionMap would index past the map's end).  Runs that
// fall short leave the rest of a new map at its initial Forward, as several summaries of the reference's own tests do (5M3D5S with
// 6F:1S:2R); a read's own runs never fall short.
PISCES_HD inline int32_t summary_direction(int64_t cs, int64_t ce, const uint8_t* op, const uint32_t* len, int32_t n_cigar, const uint8_t* run_type,
                                           const uint32_t* run_len, int32_t n_runs, int64_t preceding, int64_t trailing)
{
    const bool first_is_i = n_cigar > 0 && op[0] == 'I', last_is_i = n_cigar > 0 && op[n_cigar - 1] == 'I';
    if (!spans(cs, ce, first_is_i, last_is_i, preceding, trailing)) return kDropped;
    if (n_runs == 1) return run_type[0];
    int64_t total = 0;
    for (int32_t r = 0; r < n_runs; r++) total += run_len[r];
    if (total > read_span(op, len, n_cigar)) return kMalformed;
    auto dir_at = [&](int64_t i) -> int32_t {
        int64_t at = 0;
        for (int32_t r = 0; r < n_runs; r++) {
            at += run_len[r];
            if (i < at) return run_type[r];
        }
        return 0;
    };
    return walk_direction(cs, op, len, n_cigar, dir_at, preceding, trailing);
}

}  // namespace exact
}  // namespace pisces
