// surface_vqr.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// VariantQualityRecalibration over called-allele rows: the counting pass and the update pass on device-resident rows (vqr_kernels.hip.h),
// the counting pass over host rows and the two tables between them on the host (vqr.h).  Entries without a handle leave their message where
// a failed pisces_hip_create leaves its own: pisces_hip_last_error(NULL).

static int32_t vqr_check_options(PiscesHip* h, const char* what, const PiscesVqrOptions* opts)
{
    if (!opts) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null options");
    if (opts->extent_of_edge_region < 0 || opts->extent_of_edge_region > vqr::kMaxExtent)
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": extent_of_edge_region " + std::to_string(opts->extent_of_edge_region) + " is outside 0.." +
                                                 std::to_string(vqr::kMaxExtent));
    return PISCES_OK;
}

static int32_t vqr_check_range(PiscesHip* h, const char* what, int64_t n, int64_t lo, int64_t hi)
{
    if (n < 0) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": negative row count");
    if (lo < 0 || hi < lo || hi > n)
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are not inside [0, " + std::to_string(n) + "]");
    return PISCES_OK;
}

int32_t pisces_hip_vqr_default_options(PiscesVqrOptions* opts)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    if (!opts) return fail(nullptr, PISCES_E_INVALID_ARG, "vqr_default_options: null options");
    std::memset(opts, 0, sizeof(*opts));
    opts->do_basic_checks = 1;               // VQROptions.cs: DoBasicChecks = true
    opts->do_amplicon_position_checks = 0;   // DoAmpliconPositionChecks = false
    opts->extent_of_edge_region = 4;         // ExtentofEdgeRegion
    opts->loci_count = -1;                   // LociCount
    opts->base_q_noise = 20;                 // BamFilterParams.MinimumBaseCallQuality
    opts->filter_qscore = 30;                // VariantCallingParams.MinimumVariantQScoreFilter
    opts->max_qscore = 100;                  // MaxQScore
    opts->z_factor = 2;                      // ZFactor
    opts->alignment_warning_threshold = 10;  // AlignmentWarningThreshold
    return PISCES_OK;
    });
}

int32_t pisces_hip_vqr_count(const PiscesVqrOptions* opts, const PiscesCalledAllele* recs, int64_t n, int64_t lo, int64_t hi, PiscesVqrCounts* counts,
                             uint8_t* suspect)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    int32_t rc = vqr_check_options(nullptr, "vqr_count", opts);
    if (rc != PISCES_OK) return rc;
    if (!counts || (n > 0 && !recs)) return fail(nullptr, PISCES_E_INVALID_ARG, "vqr_count: null argument");
    rc = vqr_check_range(nullptr, "vqr_count", n, lo, hi);
    if (rc != PISCES_OK) return rc;
    const bool edges = opts->do_amplicon_position_checks != 0;
    if (edges && !suspect) return fail(nullptr, PISCES_E_INVALID_ARG, "vqr_count: do_amplicon_position_checks needs the suspect bytes");
    for (int64_t i = lo; i < hi; i++) {
        const uint32_t w60 = vqr::w60_of(recs[i].filter_bits, recs[i].info);
        const int32_t cat = vqr::count_category(w60);
        counts[0].num_possible_variants++;
        if (cat != vqr::kReference) counts[0].by_category[cat]++;
        if (!edges) continue;
        const bool edge = vqr::at_edge(i, recs[i].position, recs[i].total_coverage, opts->extent_of_edge_region, [&](int64_t g, int32_t* p, int32_t* c) {
            if (g < 0 || g >= n) return false;
            *p = recs[g].position;
            *c = recs[g].total_coverage;
            return true;
        });
        const bool is_suspect = edge && cat != vqr::kReference;
        if (edge) counts[1].num_possible_variants++;
        if (is_suspect) counts[1].by_category[cat]++;
        suspect[i] = is_suspect ? 1 : 0;
    }
    return PISCES_OK;
    });
}

int32_t pisces_hip_vqr_tables(const PiscesVqrOptions* opts, const PiscesVqrCounts* counts, PiscesVqrTables* tables)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    const int32_t rc = vqr_check_options(nullptr, "vqr_tables", opts);
    if (rc != PISCES_OK) return rc;
    if (!counts || !tables) return fail(nullptr, PISCES_E_INVALID_ARG, "vqr_tables: null argument");
    vqr::Counts c[2];
    for (int k = 0; k < 2; k++) {
        for (int32_t j = 0; j < vqr::kCategories; j++) c[k].by_category[j] = (double)counts[k].by_category[j];
        c[k].num_possible = (double)counts[k].num_possible_variants;
        if (opts->loci_count > 0) c[k].num_possible = (double)opts->loci_count;   // ForceTotalPossibleMutations, both (SignatureSorter.cs:78-82)
        c[k].removed = false;
    }
    std::memset(tables, 0, sizeof(*tables));
    if (opts->do_basic_checks) tables->basic_mask = vqr::rates(c[0], opts->base_q_noise, opts->z_factor, tables->basic);
    if (opts->do_amplicon_position_checks) tables->edge_mask = vqr::rates(c[1], opts->base_q_noise, opts->z_factor, tables->edge);
    if (opts->do_basic_checks && opts->do_amplicon_position_checks) {   // QualityRecalibration.cs:124-125
        tables->general_edge_risk_increase = vqr::edge_risk(c[0], c[1], tables->edge_risk);
        tables->has_edge_risk = 1;
    }
    return PISCES_OK;
    });
}

int32_t pisces_hip_vqr_count_device(PiscesHip* h, const PiscesVqrOptions* opts, const PiscesCalledAllele* d_recs, int64_t n, const int32_t* d_count,
                                    int64_t lo, int64_t hi, PiscesVqrCounts* d_counts, uint8_t* d_suspect, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    int32_t rc = vqr_check_options(h, "vqr_count_device", opts);
    if (rc != PISCES_OK) return rc;
    if (!d_counts || (n > 0 && !d_recs)) return fail(h, PISCES_E_INVALID_ARG, "vqr_count_device: null argument");
    rc = vqr_check_range(h, "vqr_count_device", n, lo, hi);
    if (rc != PISCES_OK) return rc;
    const bool edges = opts->do_amplicon_position_checks != 0;
    if (edges && !d_suspect) return fail(h, PISCES_E_INVALID_ARG, "vqr_count_device: do_amplicon_position_checks needs the suspect bytes");
    const int64_t blocks = (hi - lo + vqrdev::kBlock - 1) / vqrdev::kBlock;
    if (blocks > 0x7fffffffll) return fail(h, PISCES_E_INVALID_ARG, "vqr_count_device: more rows than one launch holds");
    if (blocks == 0) return PISCES_OK;
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    hipLaunchKernelGGL(vqrdev::vqr_count_kernel, dim3((unsigned)blocks), dim3(vqrdev::kBlock), 0, s, d_recs, n, d_count, lo, hi,
                       edges ? opts->extent_of_edge_region : -1, reinterpret_cast<unsigned long long*>(d_counts), d_suspect);
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}

int32_t pisces_hip_vqr_apply_device(PiscesHip* h, const PiscesVqrOptions* opts, const PiscesVqrTables* tables, PiscesCalledAllele* d_recs, int64_t n,
                                    const int32_t* d_count, const uint8_t* d_suspect, int64_t* d_n_changed, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    const int32_t rc = vqr_check_options(h, "vqr_apply_device", opts);
    if (rc != PISCES_OK) return rc;
    if (!tables || (n > 0 && !d_recs)) return fail(h, PISCES_E_INVALID_ARG, "vqr_apply_device: null argument");
    if (n < 0) return fail(h, PISCES_E_INVALID_ARG, "vqr_apply_device: negative row count");
    vqr::ApplyTables T;
    std::memset(&T, 0, sizeof(T));
    T.basic_mask = opts->do_basic_checks ? (tables->basic_mask & 0xfffu) : 0u;
    T.edge_mask = opts->do_amplicon_position_checks ? (tables->edge_mask & 0xfffu) : 0u;
    if (T.edge_mask && !d_suspect) return fail(h, PISCES_E_INVALID_ARG, "vqr_apply_device: do_amplicon_position_checks needs the suspect bytes");
    if (T.edge_mask && !tables->has_edge_risk)
        return fail(h, PISCES_E_INVALID_ARG, "vqr_apply_device: an edge table without the edge-risk table (made with both checks on): the reference reads a "
                                             "null EdgeRiskLookupTable there");
    for (int32_t c = 0; c < vqr::kSnvCategories; c++) {
        T.basic[c] = tables->basic[c];
        T.edge_risk[c] = tables->edge_risk[c];
        T.basic_err[c] = vqr::q_to_p((double)tables->basic[c]);
        T.edge_risk_err[c] = vqr::q_to_p((double)tables->edge_risk[c]);
    }
    T.max_qscore = opts->max_qscore;
    T.filter_qscore = opts->filter_qscore;
    T.ln10 = std::log(10.0);
    const int64_t blocks = (n + vqrdev::kBlock - 1) / vqrdev::kBlock;
    if (blocks > 0x7fffffffll) return fail(h, PISCES_E_INVALID_ARG, "vqr_apply_device: more rows than one launch holds");
    if (blocks == 0 || (T.basic_mask | T.edge_mask) == 0) return PISCES_OK;   // no category in a table: no row changes
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    hipLaunchKernelGGL(vqrdev::vqr_apply_kernel, dim3((unsigned)blocks), dim3(vqrdev::kBlock), 0, s, d_recs, n, d_count, d_suspect, T,
                       reinterpret_cast<unsigned long long*>(d_n_changed));
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}
