// surface_indel_repeat.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// FilterType.IndelRepeatLength's switch.  The pass itself is indel_repeat_kernel behind call_spanning_kernel in span_device_pass
// (surface_flush.inc.h); the decision's host form is indel_repeat.cpp.

int32_t pisces_hip_set_indel_repeat_filter(PiscesHip* h, int32_t threshold)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    if (threshold < 0) return fail(h, PISCES_E_INVALID_ARG, "set_indel_repeat_filter: " + std::to_string(threshold) + " is no threshold (0 = off, or a repeat length above 0)");
    h->indel_repeat_threshold = threshold;
    return PISCES_OK;
    });
}
