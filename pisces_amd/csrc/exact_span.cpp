// exact_span.cpp — the host form of exact_span.h: pisces_hip_exact_span_direction, the per-read decision of CoverageMethod.Exact for a
// caller that holds a read's coverage summary itself.  Pure host code, no device, no handle.
#include "exact_span.h"

#include "../../include/pisces_hip.h"

extern "C" {

int32_t pisces_hip_exact_span_direction(int32_t cs, int32_t ce, const uint8_t* cigar_op, const uint32_t* cigar_len, int32_t n_cigar, const uint8_t* dir_run_type,
                                        const uint32_t* dir_run_len, int32_t n_runs, int32_t preceding, int32_t trailing, int32_t is_insertion)
{
    (void)is_insertion;   // (CalculateSpanning takes it and never reads it)
    if (n_cigar < 0 || n_runs < 0 || (n_cigar > 0 && (!cigar_op || !cigar_len)) || (n_runs > 0 && (!dir_run_type || !dir_run_len))) return pisces::exact::kMalformed;
    for (int32_t r = 0; r < n_runs; r++)
        if (dir_run_type[r] > 2) return pisces::exact::kMalformed;
    return pisces::exact::summary_direction(cs, ce, cigar_op, cigar_len, n_cigar, dir_run_type, dir_run_len, n_runs, preceding, trailing);
}

}  // extern "C"
