// indel_repeat_kernels.hip.h — FilterType.IndelRepeatLength on the streaming surface (pisces_hip_set_indel_repeat_filter, FILTER R<n>).
// AlleleProcessor.ApplyFilters asks ComputeIndelRepeatLength for every variant allele (AlleleProcessor.cs:52-57); only insertions and
// deletions can have a length above 0, and they are the candidates of call_spanning_kernel: a pass of its own over that kernel's records,
// enqueued behind it on a handle whose threshold is above 0 and on no other.  The decision is indel_repeat.h, the source the host entry uses.
#pragma once
#include "indel_repeat.h"
#include "kernels.hip.h"

namespace pisces {

// One lane per candidate of the pass call_spanning_kernel has just made (the same cands / alleles / records / callable arrays).  A record
// is there for every candidate when every_record is set, else for the callable ones.  A handful of rows, a window of at most 100 reference
// bases each: nothing shared, nothing atomic; the only store is the 16-bit filter word of a flagged row.
__global__ __launch_bounds__(64) void indel_repeat_kernel(const DevCandidate* __restrict__ cands, int32_t n, const uint8_t* __restrict__ alleles,
                                                          const uint8_t* __restrict__ ref, int64_t ref_len /* ref[i] = position i+1 */,
                                                          const uint8_t* __restrict__ callable, int32_t every_record, int32_t threshold,
                                                          PiscesCalledAllele* __restrict__ records)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int32_t category = cands[i].category;
    if (category != PISCES_CAT_INSERTION && category != PISCES_CAT_DELETION) return;
    if (!every_record && !callable[i]) return;
    const DevCandidate c = cands[i];
    const uint8_t* ra = alleles + c.allele_off;
    const int32_t length = indel_repeat::length(category, c.position, ra, c.ref_len, ra + c.ref_len, c.alt_len, ref, ref_len);
    // indelRepeatFilter <= indelRepeatLength (:55); where the reference's Substring throws (a candidate beyond the chromosome) nothing is flagged
    if (length >= threshold) records[i].filter_bits = (uint16_t)(records[i].filter_bits | (1u << PISCES_FILTER_INDEL_REPEAT_LENGTH));
}

}  // namespace pisces
