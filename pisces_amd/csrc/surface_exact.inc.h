// surface_exact.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// CoverageMethod.Exact's entries: the switch of the handle and what a host needs of IAlleleSource.GetSpanningReadSummaries.  The summaries
// live in the read store (exact_store_summaries, surface_store.inc.h); the flush's passes are exact_candidate_coverage in span_collapse and
// span_device_pass (surface_flush.inc.h); the per-read decision's host form is exact_span.cpp.

// what cannot go together with Exact; nullptr: nothing
static const char* exact_refusal(const PiscesHip* h)
{
    if (h->cfg.noise_model == PISCES_NOISE_WINDOW) return "NoiseModel.Window: the Exact calculator's own sum of base qualities (ExactCoverageCalculator.cs:50-57) is not carried";
    if (!h->forced.empty()) return "forced alleles are set";
    if (h->own_lo != 1 || h->own_hi != 0x7FFFFFFF) return "an owned range is set (pisces_hip_set_owned_range): a shard's halo is cut by aligned span, not by clip-adjusted span";
    if (h->read_path != 1) return "PISCES_HIP_READ_PATH=log: observation tuples have no reads";
    return nullptr;
}

int32_t pisces_hip_set_coverage_method(PiscesHip* h, int32_t method)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    if (method != PISCES_COVERAGE_APPROXIMATE && method != PISCES_COVERAGE_EXACT)
        return fail(h, PISCES_E_INVALID_ARG, "set_coverage_method: " + std::to_string(method) + " is no CoverageMethod (PISCES_COVERAGE_APPROXIMATE, PISCES_COVERAGE_EXACT)");
    if (h->stats[2] > 0 || !store_is_empty(h) || h->log_ub > 0 || !h->blocks.empty())
        return fail(h, PISCES_E_STATE, "set_coverage_method: reads have been added already");
    if (method == PISCES_COVERAGE_EXACT) {
        const char* why = exact_refusal(h);
        if (why) return fail(h, PISCES_E_UNSUPPORTED, std::string("set_coverage_method: ") + why);
    }
    h->exact_on = method == PISCES_COVERAGE_EXACT;
    return PISCES_OK;
    });
}

int32_t pisces_hip_get_spanning_read_counts(PiscesHip* h, int32_t preceding, int32_t trailing, int32_t is_insertion, int32_t* out)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    (void)is_insertion;   // (ExactCoverageCalculator.CalculateSpanning takes it and never reads it)
    if (!out) return fail(h, PISCES_E_INVALID_ARG, "get_spanning_read_counts: null output");
    if (!h->exact_on) return fail(h, PISCES_E_STATE, "get_spanning_read_counts: the handle keeps no read summaries (pisces_hip_set_coverage_method, PISCES_COVERAGE_EXACT)");
    out[0] = out[1] = out[2] = 0;
    if (preceding > trailing) return PISCES_OK;
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    const int32_t span[2] = {preceding, trailing};
    int32_t counts[4] = {0, 0, 0, 0}, failed = -1;
    { int32_t rc = exact_launch(h, span, 1, counts, &failed); if (rc) return rc; }
    if (failed >= 0)
        return fail(h, PISCES_E_INVALID_ARG, "get_spanning_read_counts: Invalid indices -1--1: a read of several directions has no base at or before " + std::to_string(preceding) +
                                                 " and none at or behind " + std::to_string(trailing) + "; the reference throws here");
    out[0] = counts[0]; out[1] = counts[1]; out[2] = counts[2];
    return PISCES_OK;
    });
}
