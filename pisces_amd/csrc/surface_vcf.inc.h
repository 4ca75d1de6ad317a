// surface_vcf.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// pisces_hip_format_vcf_device: VCF body lines from device-resident rows (vcf_kernels.hip.h), stream-ordered behind whatever made them.

int32_t pisces_hip_format_vcf_device(PiscesHip* h, const PiscesVcfConfig* cfg, const char* chrom, const PiscesCalledAllele* d_recs, int64_t n,
                                     const int32_t* d_count, const int32_t* d_cand_index, const PiscesCandidate* d_cands, const uint8_t* d_alleles,
                                     const PiscesGenotypePosteriors* d_gp, char* d_text, int64_t text_capacity, int64_t* d_line_offsets,
                                     int64_t* d_text_bytes, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    if (!cfg || !chrom || !d_text_bytes) return fail(h, PISCES_E_INVALID_ARG, "format_vcf_device: null argument");
    if (n < 0 || text_capacity < 0) return fail(h, PISCES_E_INVALID_ARG, "format_vcf_device: negative size");
    if ((n > 0 && !d_recs) || (text_capacity > 0 && !d_text)) return fail(h, PISCES_E_INVALID_ARG, "format_vcf_device: null device pointer");
    if (cfg->crush)
        return fail(h, PISCES_E_UNSUPPORTED, "format_vcf_device: crushed lines (PiscesVcfConfig.crush) merge the rows of a position; pisces_hip_format_vcf writes them");
    const size_t chrom_len = std::strlen(chrom);
    if (chrom_len > (size_t)vcfdev::kMaxChrom)
        return fail(h, PISCES_E_UNSUPPORTED, "format_vcf_device: chrom is longer than 1024 bytes (it travels in the kernel arguments)");
    const int decimals = pisces_vcf_frequency_decimals(cfg);
    if (decimals > vcfdev::kMaxDecimals)
        return fail(h, PISCES_E_UNSUPPORTED, "format_vcf_device: frequency thresholds below 1e-7 ask for more than 7 VF decimals, which the device's 128-bit "
                                             "arithmetic does not hold for a Double; pisces_hip_format_vcf writes them");
    vcfdev::VcfArgs A;
    std::memset(&A, 0, sizeof(A));
    A.recs = d_recs;
    A.n = n;
    A.d_count = d_count;
    A.cand_index = d_cand_index;
    A.cands = d_cands;
    A.alleles = d_alleles;
    A.gp = d_gp;
    A.text = d_text;
    A.capacity = text_capacity;
    A.line_offsets = d_line_offsets;
    A.text_bytes = d_text_bytes;
    A.variant_quality_filter = cfg->variant_quality_filter;
    A.rmxn_max_repeat_length = cfg->rmxn_max_repeat_length;
    A.rmxn_min_repetitions = cfg->rmxn_min_repetitions;
    A.noise_level = cfg->noise_level;
    A.output_sb_nl = cfg->output_strand_bias_and_noise_level;
    A.output_nc = cfg->output_no_call_fraction;
    A.noise_level_from_records = cfg->noise_level_from_records;
    A.freq_decimals = decimals;
    A.chrom_len = (int32_t)chrom_len;
    std::memcpy(A.chrom, chrom, chrom_len);
    std::string format = "GT:GQ:AD:DP:VF";
    if (cfg->output_strand_bias_and_noise_level) format += ":NL:SB";
    if (cfg->output_no_call_fraction) format += ":NC";
    A.format_len = (int32_t)format.size();
    std::memcpy(A.format, format.data(), format.size());
    if (cfg->variant_quality_filter >= 0) {
        const std::string q = "q" + std::to_string(cfg->variant_quality_filter);
        A.qname_len = (int32_t)q.size();
        std::memcpy(A.qname, q.data(), q.size());
    }
    if (cfg->rmxn_max_repeat_length >= 0 && cfg->rmxn_min_repetitions >= 0) {
        const std::string r = "R" + std::to_string(cfg->rmxn_max_repeat_length) + "x" + std::to_string(cfg->rmxn_min_repetitions);
        A.rname_len = (int32_t)r.size();
        std::memcpy(A.rname, r.data(), r.size());
    }
    if (cfg->indel_repeat_filter > 0) {
        const std::string r = "R" + std::to_string(cfg->indel_repeat_filter);
        A.iname_len = (int32_t)r.size();
        std::memcpy(A.iname, r.data(), r.size());
    }
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    const int64_t chunks = (n + vcfdev::kRowsPerChunk - 1) / vcfdev::kRowsPerChunk;
    if (chunks > 0x7fffffffll) return fail(h, PISCES_E_INVALID_ARG, "format_vcf_device: more rows than one launch holds");
    // the scratch grows only: an earlier call of this handle may still read the buffer that growing gives back, so that call is waited for
    // (calls of one handle are stream-ordered with respect to each other, include/pisces_hip.h; a handle that has seen a caller's stream
    // waits for the device, since the earlier call may sit on another stream than this one)
    if ((size_t)n > h->d_vcf_len.cap || (size_t)chunks > h->d_vcf_chunk.cap || !h->d_vcf_ctrl.p) {
        if (h->foreign_stream_ever) PISCES_HIP_CHECK(h, hipDeviceSynchronize());
        else PISCES_HIP_CHECK(h, hipStreamSynchronize(s));
        PISCES_HIP_CHECK(h, h->d_vcf_len.reserve((size_t)n + 1));
        PISCES_HIP_CHECK(h, h->d_vcf_chunk.reserve((size_t)chunks + 1));
        PISCES_HIP_CHECK(h, h->d_vcf_ctrl.reserve(2));
    }
    A.row_len = h->d_vcf_len.p;
    A.chunk_off = h->d_vcf_chunk.p;
    A.ctrl = h->d_vcf_ctrl.p;
    PISCES_HIP_CHECK(h, hipMemsetAsync(A.ctrl, 0xff, sizeof(unsigned long long), s));
    if (chunks > 0) hipLaunchKernelGGL(vcfdev::vcf_length_kernel, dim3((unsigned)chunks), dim3(vcfdev::kRowsPerChunk), 0, s, A);
    hipLaunchKernelGGL(vcfdev::vcf_scan_kernel, dim3(1), dim3(1024), 0, s, A, chunks);
    if (chunks > 0) hipLaunchKernelGGL(vcfdev::vcf_write_kernel, dim3((unsigned)chunks), dim3(vcfdev::kRowsPerChunk), 0, s, A);
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}
