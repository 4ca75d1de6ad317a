// surface_venn.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// VennVcf's consensus of two probe pools over called-allele rows: on device-resident rows (venn_kernels.hip.h) and over host rows, both
// through venn::walk_group (venn.h) with the two scores of VennMath.  Entries without a handle leave their message where a failed
// pisces_hip_create leaves its own: pisces_hip_last_error(NULL).

static int32_t venn_check_options(PiscesHip* h, const char* what, const PiscesVennOptions* opts)
{
    if (!opts) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null options");
    const float thresholds[3] = {opts->min_frequency, opts->min_frequency_filter, opts->pool_bias_threshold};
    const char* names[3] = {"min_frequency", "min_frequency_filter", "pool_bias_threshold"};
    for (int k = 0; k < 3; k++)
        if (!(thresholds[k] >= 0.0f && thresholds[k] <= 1.0f))
            return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": " + names[k] + " " + std::to_string(thresholds[k]) + " is outside [0, 1]");
    if (opts->combine_qscore_method != 0 && opts->combine_qscore_method != 1)
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": combine_qscore_method " + std::to_string(opts->combine_qscore_method) +
                                                 " is neither 0 (pool and recalculate) nor 1 (take min)");
    return PISCES_OK;
}

static int32_t venn_check_rows(PiscesHip* h, const char* what, const char* pool, const PiscesVennRows* r)
{
    if (!r) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null pool " + pool);
    if (r->n < 0) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": pool " + pool + " has a negative row count");
    if (r->n > 0 && !r->recs) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": pool " + pool + " has rows and a null recs");
    if (r->cand_index && (!r->cands || !r->alleles))
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": pool " + pool + " has a cand_index without its candidates and allele bytes");
    return PISCES_OK;
}

static int32_t venn_check_out(PiscesHip* h, const char* what, const PiscesVennOut* out)
{
    if (!out) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null out");
    if (!out->n_out) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null n_out");
    if (out->row_capacity < 0 || out->cand_capacity < 0 || out->allele_capacity < 0)
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": negative capacity");
    if ((out->row_capacity > 0 && (!out->recs || !out->cand_index)) || (out->cand_capacity > 0 && !out->cands) || (out->allele_capacity > 0 && !out->alleles))
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": a capacity above 0 with a null output array");
    return PISCES_OK;
}

int32_t pisces_hip_venn_default_options(PiscesVennOptions* opts)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    if (!opts) return fail(nullptr, PISCES_E_INVALID_ARG, "venn_default_options: null options");
    std::memset(opts, 0, sizeof(*opts));
    opts->min_frequency = 0.01f;          // VariantCallingParameters.MinimumFrequency
    opts->min_frequency_filter = 0.01f;   // MinimumFrequencyFilter: unset, raised to MinimumFrequency
    opts->pool_bias_threshold = 0.5f;     // SampleAggregationParameters.ProbePoolBiasThreshold
    opts->min_coverage = 10;              // MinimumCoverage
    opts->max_variant_qscore = 100;       // MaximumVariantQScore
    opts->combine_qscore_method = 0;      // HowToCombineQScore = CombinePoolsAndReCalculate
    return PISCES_OK;
    });
}

int32_t pisces_hip_venn_combine(const PiscesVennOptions* opts, const PiscesCalledAllele* a, const PiscesCalledAllele* b, int32_t comparison_case,
                                PiscesCalledAllele* row_out, PiscesConsensusInfo* info_out, int32_t* vq_ab)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    const int32_t rc = venn_check_options(nullptr, "venn_combine", opts);
    if (rc != PISCES_OK) return rc;
    if (!a && !b) return fail(nullptr, PISCES_E_INVALID_ARG, "venn_combine: both members are null");
    if (!row_out) return fail(nullptr, PISCES_E_INVALID_ARG, "venn_combine: null row_out");
    if (comparison_case > venn::kCanNotCombine) return fail(nullptr, PISCES_E_INVALID_ARG, "venn_combine: unknown comparison case");
    const int32_t natural = venn::comparison_case(a != nullptr, a ? a->info : 0u, b != nullptr, b ? b->info : 0u);
    const int32_t cmp = comparison_case < 0 ? natural : comparison_case;
    if ((!a || !b) && cmp != venn::kCanNotCombine) return fail(nullptr, PISCES_E_INVALID_ARG, "venn_combine: a missing member can only be CanNotCombine");
    const VennMath math = {std::log(10.0)};
    venn::Combined c = venn::combine(a, b, cmp, *opts, math, a ? (int32_t)PISCES_INFO_REF(a->info) : 0, b ? (int32_t)PISCES_INFO_REF(b->info) : 0);
    c.info.row_a = a ? 0 : -1;
    c.info.row_b = b ? 0 : -1;
    *row_out = c.row;
    if (info_out) *info_out = c.info;
    if (vq_ab) { vq_ab[0] = c.vq_a; vq_ab[1] = c.vq_b; }
    return PISCES_OK;
    });
}

namespace {
struct VennHostCount {
    void row(int64_t, const PiscesCalledAllele&, const PiscesConsensusInfo&) {}
    void cand(int64_t, int64_t, int64_t, const PiscesCandidate&, const uint8_t*) {}
    void no_cand(int64_t) {}
    void venn(int, int64_t, uint8_t) {}
};
struct VennHostEmit {
    const PiscesVennOut& out;
    int64_t row_base, cand_base, byte_base;
    void row(int64_t slot, const PiscesCalledAllele& r, const PiscesConsensusInfo& info)
    {
        venn::store_row(out.recs + row_base + slot, r);
        if (out.info) std::memcpy(out.info + row_base + slot, &info, sizeof(info));
    }
    void cand(int64_t slot, int64_t cslot, int64_t byte_off, const PiscesCandidate& c, const uint8_t* bytes)
    {
        out.cand_index[row_base + slot] = (int32_t)(cand_base + cslot);
        PiscesCandidate o = c;
        o.allele_offset = byte_base + byte_off;
        out.cands[cand_base + cslot] = o;
        std::memcpy(out.alleles + byte_base + byte_off, bytes, (size_t)c.ref_len + (size_t)c.alt_len);
    }
    void no_cand(int64_t slot) { out.cand_index[row_base + slot] = -1; }
    void venn(int pool, int64_t i, uint8_t cls)
    {
        uint8_t* v = pool ? out.venn_b : out.venn_a;
        if (v) v[i] = cls;
    }
};
venn::Pool venn_host_pool(const PiscesVennRows& r)
{
    venn::Pool p;
    p.recs = r.recs;
    p.n = r.n;
    if (r.count) p.n = *r.count < 0 ? 0 : std::min<int64_t>(r.n, *r.count);
    p.cand_index = r.cand_index;
    p.cands = r.cands;
    p.alleles = r.alleles;
    return p;
}
// DoPairwiseVenn's walk (VennVcf.cs:129-266): the lower first position of the two backlogs, the rows of it from both pools
void venn_host_walk(const venn::Pool& A, const venn::Pool& B, const PiscesVennOptions& opts, const VennMath& math, bool emit, const PiscesVennOut* out,
                    venn::GroupCounts& total)
{
    total = {0, 0, 0};
    int64_t ia = 0, ib = 0;
    while (ia < A.n || ib < B.n) {
        const bool take_a = ia < A.n && (ib >= B.n || A.recs[ia].position <= B.recs[ib].position);
        const int32_t position = take_a ? A.recs[ia].position : B.recs[ib].position;
        const int64_t a1 = (ia < A.n && A.recs[ia].position == position) ? venn::group_end(A.recs, A.n, ia) : ia;
        const int64_t b1 = (ib < B.n && B.recs[ib].position == position) ? venn::group_end(B.recs, B.n, ib) : ib;
        venn::GroupCounts n;
        if (emit) {
            VennHostEmit sink = {*out, total.rows, total.cands, total.bytes};
            n = venn::walk_group(A, ia, a1, B, ib, b1, opts, math, sink);
        } else {
            VennHostCount sink;
            n = venn::walk_group(A, ia, a1, B, ib, b1, opts, math, sink);
        }
        total.rows += n.rows;
        total.cands += n.cands;
        total.bytes += n.bytes;
        ia = a1;
        ib = b1;
    }
}
}  // namespace

int32_t pisces_hip_venn_consensus(const PiscesVennOptions* opts, const PiscesVennRows* a, const PiscesVennRows* b, const PiscesVennOut* out)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    int32_t rc = venn_check_options(nullptr, "venn_consensus", opts);
    if (rc == PISCES_OK) rc = venn_check_rows(nullptr, "venn_consensus", "A", a);
    if (rc == PISCES_OK) rc = venn_check_rows(nullptr, "venn_consensus", "B", b);
    if (rc == PISCES_OK) rc = venn_check_out(nullptr, "venn_consensus", out);
    if (rc != PISCES_OK) return rc;
    const venn::Pool A = venn_host_pool(*a), B = venn_host_pool(*b);
    for (int pool = 0; pool < 2; pool++) {   // "Vcf needs to be ordered." (VennVcf.cs:401-404)
        const venn::Pool& P = pool ? B : A;
        for (int64_t i = 1; i < P.n; i++)
            if (P.recs[i].position < P.recs[i - 1].position) {
                out->n_out[0] = PISCES_E_INVALID_ARG;
                out->n_out[1] = pool;
                out->n_out[2] = i;
                return fail(nullptr, PISCES_E_INVALID_ARG, std::string("venn_consensus: pool ") + (pool ? "B" : "A") + " is not sorted by position at row " + std::to_string(i));
            }
    }
    const VennMath math = {std::log(10.0)};
    venn::GroupCounts total;
    venn_host_walk(A, B, *opts, math, false, out, total);
    out->n_out[0] = total.rows;
    out->n_out[1] = total.cands;
    out->n_out[2] = total.bytes;
    if (total.rows > out->row_capacity || total.cands > out->cand_capacity || total.bytes > out->allele_capacity)
        return fail(nullptr, PISCES_E_BUFFER_TOO_SMALL, "venn_consensus: " + std::to_string(total.rows) + " rows, " + std::to_string(total.cands) + " candidates and " +
                                                            std::to_string(total.bytes) + " allele bytes do not fit the capacities");
    venn_host_walk(A, B, *opts, math, true, out, total);
    return PISCES_OK;
    });
}

int32_t pisces_hip_venn_consensus_device(PiscesHip* h, const PiscesVennOptions* opts, const PiscesVennRows* a, const PiscesVennRows* b,
                                         const PiscesVennOut* out, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    int32_t rc = venn_check_options(h, "venn_consensus_device", opts);
    if (rc == PISCES_OK) rc = venn_check_rows(h, "venn_consensus_device", "A", a);
    if (rc == PISCES_OK) rc = venn_check_rows(h, "venn_consensus_device", "B", b);
    if (rc == PISCES_OK) rc = venn_check_out(h, "venn_consensus_device", out);
    if (rc != PISCES_OK) return rc;
    if (((uintptr_t)a->recs | (uintptr_t)b->recs | (uintptr_t)out->recs | (uintptr_t)out->info) & 15u)
        return fail(h, PISCES_E_INVALID_ARG, "venn_consensus_device: rows and info are read and written 16 bytes at a time, a pointer is not 16-byte aligned");
    venndev::Args K;
    std::memset(&K, 0, sizeof(K));
    K.a = *a;
    K.b = *b;
    K.out = *out;
    K.opts = *opts;
    K.math.ln10 = std::log(10.0);
    K.chunks_a = (a->n + venndev::kBlock - 1) / venndev::kBlock;
    K.chunks_b = (b->n + venndev::kBlock - 1) / venndev::kBlock;
    const int64_t chunks = K.chunks_a + K.chunks_b, rows = a->n + b->n;
    if (chunks > 0x7fffffffll) return fail(h, PISCES_E_INVALID_ARG, "venn_consensus_device: more rows than one launch holds");
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    // the scratch grows only; an earlier call of this handle may still read what growing gives back (as pisces_hip_format_vcf_device)
    if ((size_t)rows * 3 > h->d_venn_prefix.cap || (size_t)chunks * 3 > h->d_venn_chunk.cap || !h->d_venn_ctrl.p) {
        if (h->foreign_stream_ever) PISCES_HIP_CHECK(h, hipDeviceSynchronize());
        else PISCES_HIP_CHECK(h, hipStreamSynchronize(s));
        PISCES_HIP_CHECK(h, h->d_venn_prefix.reserve((size_t)rows * 3 + 3));
        PISCES_HIP_CHECK(h, h->d_venn_chunk.reserve((size_t)chunks * 3 + 3));
        PISCES_HIP_CHECK(h, h->d_venn_ctrl.reserve(8));
    }
    K.prefix = h->d_venn_prefix.p;
    K.chunk = h->d_venn_chunk.p;
    K.ctrl = h->d_venn_ctrl.p;
    PISCES_HIP_CHECK(h, hipMemsetAsync(K.ctrl, 0xff, sizeof(unsigned long long), s));
    if (chunks > 0) hipLaunchKernelGGL(venndev::venn_count_kernel, dim3((unsigned)chunks), dim3(venndev::kBlock), 0, s, K);
    hipLaunchKernelGGL(venndev::venn_scan_kernel, dim3(1), dim3(1024), 0, s, K);
    if (chunks > 0) hipLaunchKernelGGL(venndev::venn_emit_kernel, dim3((unsigned)chunks), dim3(venndev::kBlock), 0, s, K);
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}
