// exact_kernels.hip.h — CoverageMethod.Exact on the read store (pisces_hip_set_coverage_method, -coveragemethod exact).
// IAlleleSource.GetSpanningReadSummaries + ExactCoverageCalculator.CalculateSpanning are a search plus a predicate over the reads the store
// holds: the reference keeps a List<ReadCoverageSummary> per position of the block of a read's clip-adjusted end and scans, per allele,
// the lists of trailing + 2 * read length positions (RegionStateManager.cs:212-219, :234-254); here an exact handle keeps a 16-byte
// summary per read next to its descriptor (exact_summary_kernel, add time) and a flush counts, one wave per spanning candidate, the reads
// of every segment whose summary passes (exact_span_kernel).  The per-read decision is exact_span.h, the source the host entry uses.
#pragma once
#include "exact_span.h"
#include "store_kernels.hip.h"

namespace pisces {

struct ExactSummary {   // Read.GetCoverageSummary (Read.cs:613-622): what decides without the CIGAR
    int32_t cs, ce;     // ClipAdjustedPosition, ClipAdjustedEndPosition
    uint32_t bits;      // kExact*
    int32_t pad;
};
static_assert(sizeof(ExactSummary) == 16, "summary layout");
constexpr uint32_t kExactFirstI = 1u, kExactLastI = 2u;   // the strict first / last CIGAR operation is an insertion
constexpr uint32_t kExactMulti = 4u;                     // more than one direction run: the read's CIGAR and directions are walked
constexpr int kExactDirShift = 3;                        // the direction of a read of one run, 2 bits
constexpr int kExactBoundSpan = 0, kExactBoundLead = 1;  // a segment's bounds: the longest CE - Position and the longest Position - CS of its reads
constexpr int32_t kExactNoError = 0x7FFFFFFF;

// the summaries of an exact handle's segments, in StoreView's order (kept out of SegmentView: the flush kernels' arguments stay as they are)
struct ExactView {
    const ExactSummary* sum[kMaxSegments];
    const int32_t* bounds[kMaxSegments];
};

// One lane per read of a batch that has just joined a segment (the batch's own arrays, offsets relative to the batch).  dirs == nullptr: the
// batch carries no per-base directions (every read has the one of its flags).  l0 != nullptr: the handle has seen no read yet — read 0's
// length becomes RegionStateManager._readLength (:120-121).  extra_key[r]: the block of the read's clip-adjusted end where no aligned base of
// the read lies in it (AddReadSummary's GetBlock creates it, :216), else 0; n_extra counts them.
__global__ __launch_bounds__(256) void exact_summary_kernel(const int32_t* __restrict__ position, const uint8_t* __restrict__ flags, const int32_t* __restrict__ cigar_offset,
                                                            const uint8_t* __restrict__ cigar_op, const uint32_t* __restrict__ cigar_len, const int32_t* __restrict__ seq_offset,
                                                            const uint8_t* __restrict__ dirs, int32_t n_reads, int32_t n_ops, int32_t block_size, ExactSummary* __restrict__ out,
                                                            int32_t* __restrict__ bounds, int32_t* __restrict__ l0, int32_t* __restrict__ extra_key, int32_t* __restrict__ n_extra)
{
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    int span = 0, lead = 0;
    bool extra = false;
    if (r < n_reads) {
        const int32_t c0 = max(cigar_offset[r], 0), c1 = min(cigar_offset[r + 1], n_ops);
        const int32_t nc = max(c1 - c0, 0);
        const uint8_t* const op = cigar_op + c0;
        const uint32_t* const len = cigar_len + c0;
        const int32_t s0 = seq_offset[r], n = seq_offset[r + 1] - s0;
        const long long pos = position[r];
        const long long pre = exact::prefix_clip(op, len, nc), suf = exact::suffix_clip(op, len, nc), ref = exact::ref_span(op, len, nc);
        const long long cs = pos - pre, end = pos + ref - 1, ce = end + suf;   // Read.EndPosition = BamAlignment.EndPosition + 1
        uint32_t bits = (nc > 0 && op[0] == 'I' ? kExactFirstI : 0u) | (nc > 0 && op[nc - 1] == 'I' ? kExactLastI : 0u);
        uint32_t d0 = (flags[r] & 1) ? (uint32_t)PISCES_DIR_REVERSE : (uint32_t)PISCES_DIR_FORWARD;
        if (dirs && n > 0) {
            d0 = dirs[s0];
            bool multi = false;
            for (int i = 1; i < n; i++) multi = multi || dirs[s0 + i] != d0;
            if (multi) bits |= kExactMulti;
        }
        bits |= (d0 & 3u) << kExactDirShift;
        ExactSummary s;
        s.cs = (int32_t)max(min(cs, 0x7FFFFFFFll), -0x7FFFFFFFll);
        s.ce = (int32_t)max(min(ce, 0x7FFFFFFFll), -0x7FFFFFFFll);
        s.bits = bits;
        s.pad = 0;
        out[r] = s;
        span = (int)max(min(ce - pos, 0x7FFFFFFFll), 0ll);
        lead = (int)max(min(pre, 0x7FFFFFFFll), 0ll);
        // the block of CE against the block of the read's last aligned base (which AddAlleleCounts touches, whatever its quality)
        long long last_aligned = 0;
        {
            long long p = pos;
            for (int c = 0; c < nc; c++) {
                const bool rd = exact::op_read_span(op[c]), rf = exact::op_ref_span(op[c]);
                if (rd && rf && len[c] > 0) last_aligned = p + len[c] - 1;
                if (rf) p += len[c];
            }
        }
        const long long kce = ce >= 1 ? (ce + block_size - 1) / block_size : 0;
        const long long kla = last_aligned >= 1 ? (last_aligned + block_size - 1) / block_size : 0;
        extra = kce >= 1 && kce != kla && ce <= 0x7FFFFFFFll;
        extra_key[r] = extra ? (int32_t)kce : 0;
        if (r == 0 && l0) l0[0] = n;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        span = max(span, __shfl_xor(span, d, 64));
        lead = max(lead, __shfl_xor(lead, d, 64));
    }
    const bool any_extra = __ballot(extra) != 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (span > bounds[kExactBoundSpan]) atomicMax(&bounds[kExactBoundSpan], span);
        if (lead > bounds[kExactBoundLead]) atomicMax(&bounds[kExactBoundLead], lead);
        if (any_extra && n_extra[0] == 0) atomicOr(n_extra, 1);
    }
}

// One wave per span (spans[i] = {preceding, trailing}; preceding > trailing: not a spanning allele, the counts stay 0).  out[4 i ..]: the reads
// that span it in directions 0 / 1 / 2, and 1 in the fourth word where a read ran into exact::kNoIndices (error[0] then holds the lowest such
// span index, atomicMin; the host presets kExactNoError).  Visibility (GetSpanningReadSummaries): the block of the read's CE is still held —
// a read that was there at the last flush has CE at or above the segment's floor — and CE <= trailing + 2 * l0.
__global__ __launch_bounds__(64) void exact_span_kernel(StoreView S, ExactView X, const int32_t* __restrict__ spans, int32_t n_spans, const int32_t* __restrict__ l0,
                                                        int32_t* __restrict__ out, int32_t* __restrict__ error)
{
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= n_spans) return;
    const long long preceding = spans[2 * i], trailing = spans[2 * i + 1];
    int n_dir[3] = {0, 0, 0};
    bool failed = false;
    const long long reach = 2ll * (long long)max(l0[0], 0);
    if (preceding <= trailing && l0[0] >= 0) {
        for (int sg = 0; sg < S.n_segments; sg++) {
            const SegmentView& G = S.seg[sg];
            const ExactSummary* const sum = X.sum[sg];
            const int32_t* const bounds = X.bounds[sg];
            if (G.n_reads <= 0 || !sum || !bounds) continue;
            int lo = 0, hi = G.n_reads;
            if (G.state[kStateUnsorted] == 0) {
                // Position in [preceding - longest (CE - Position), trailing + longest leading clip]
                const long long x_lo = max(preceding - (long long)bounds[kExactBoundSpan], -0x7FFFFFFFll);
                const long long x_hi = min(trailing + (long long)bounds[kExactBoundLead] + 1, 0x7FFFFFFFll);
                wave_lower_bound2(G.desc, G.n_reads, (int)x_lo, (int)x_hi, lane, &lo, &hi);
            }
            for (int r0 = lo; r0 < hi; r0 += 64) {   // (wave-uniform trip count: the ballots below see every lane)
                const int r = r0 + lane;
                int dir = exact::kDropped;
                if (r < hi) {
                    const ExactSummary s = sum[r];
                    const bool visible = (r >= G.n_floored || s.ce >= G.floor) && (long long)s.ce <= trailing + reach;
                    if (visible && exact::spans(s.cs, s.ce, (s.bits & kExactFirstI) != 0, (s.bits & kExactLastI) != 0, preceding, trailing)) {
                        if (!(s.bits & kExactMulti) || !G.dirs) {
                            dir = (int)((s.bits >> kExactDirShift) & 3u);
                        } else {
                            const ReadDesc d = G.desc[r];
                            const ReadExt e = G.ext[r];
                            const uint8_t* const op = G.cigar_op + e.cig_off;
                            const uint32_t* const len = G.cigar_len + e.cig_off;
                            // (a read of one aligned run keeps the index of its first ALIGNED base: back to its first base)
                            long long first_base = d.aoff;
                            if (!(d.meta & kDescComplex))
                                for (int c = 0; c < e.n_cigar; c++) {
                                    if (op[c] == 'S') first_base -= (long long)len[c];
                                    else if (op[c] != 'H' && op[c] != 'P') break;
                                }
                            const uint8_t* const dirs = G.dirs + first_base;
                            dir = exact::walk_direction(s.cs, op, len, e.n_cigar, [&](long long k) -> int32_t { return (int32_t)dirs[k]; }, preceding, trailing);
                        }
                    }
                }
                n_dir[0] += __popcll(__ballot(dir == 0));
                n_dir[1] += __popcll(__ballot(dir == 1));
                n_dir[2] += __popcll(__ballot(dir == 2));
                failed = failed || __ballot(dir == exact::kNoIndices) != 0ull;
            }
        }
    }
    if (lane == 0) {
        out[4 * i] = n_dir[0];
        out[4 * i + 1] = n_dir[1];
        out[4 * i + 2] = n_dir[2];
        out[4 * i + 3] = failed ? 1 : 0;
        if (failed) atomicMin(error, i);
    }
}

}  // namespace pisces
