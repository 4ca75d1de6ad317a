// surface_nbhd.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// Scylla's neighbourhoods of phasable variants from called rows: over host rows and over device-resident rows (nbhd_kernels.hip.h), both
// through the decisions of nbhd.h.  Entries without a handle leave their message where a failed pisces_hip_create leaves its own:
// pisces_hip_last_error(NULL).

static int32_t nbhd_check(PiscesHip* h, const char* what, const PiscesNbhdCriteria* criteria, const PiscesVennRows* rows, const PiscesNbhdOut* out)
{
    const std::string w = what;
    if (!criteria) return fail(h, PISCES_E_INVALID_ARG, w + ": null criteria");
    if (!rows) return fail(h, PISCES_E_INVALID_ARG, w + ": null rows");
    if (rows->n < 0) return fail(h, PISCES_E_INVALID_ARG, w + ": negative row count");
    if (rows->n > 0x7fffffffll) return fail(h, PISCES_E_INVALID_ARG, w + ": more rows than a row index holds");
    if (rows->n > 0 && !rows->recs) return fail(h, PISCES_E_INVALID_ARG, w + ": rows and a null recs");
    if (rows->cand_index && (!rows->cands || !rows->alleles)) return fail(h, PISCES_E_INVALID_ARG, w + ": a cand_index without its candidates and allele bytes");
    if (!out) return fail(h, PISCES_E_INVALID_ARG, w + ": null out");
    if (!out->n_out) return fail(h, PISCES_E_INVALID_ARG, w + ": null n_out");
    if (out->nbhd_capacity < 0 || out->site_capacity < 0 || out->allele_capacity < 0 || out->ref_capacity < 0)
        return fail(h, PISCES_E_INVALID_ARG, w + ": negative capacity");
    if ((out->nbhd_capacity > 0 && (!out->neighbourhoods || !out->info)) || (out->site_capacity > 0 && (!out->sites || !out->site_row || !out->site_original)) ||
        (out->allele_capacity > 0 && !out->alleles) || (out->ref_capacity > 0 && !out->ref_bytes))
        return fail(h, PISCES_E_INVALID_ARG, w + ": a capacity above 0 with a null output array");
    return PISCES_OK;
}

int32_t pisces_hip_nbhd_default_criteria(PiscesNbhdCriteria* criteria)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    if (!criteria) return fail(nullptr, PISCES_E_INVALID_ARG, "nbhd_default_criteria: null criteria");
    std::memset(criteria, 0, sizeof(*criteria));
    criteria->phasing_distance = 50;              // PhasableVariantCriteria.PhasingDistance
    criteria->passing_variants_only = 1;          // PassingVariantsOnly
    criteria->het_variants_only = 0;              // HetVariantsOnly
    criteria->min_passing_variants_in_nbhd = 0;   // MinPassingVariantsInNbhd
    return PISCES_OK;
    });
}

int32_t pisces_hip_nbhd_build(const PiscesNbhdCriteria* criteria, const PiscesVennRows* rows, const uint8_t* reference, int64_t reference_length,
                              const PiscesNbhdOut* out)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    const int32_t rc = nbhd_check(nullptr, "nbhd_build", criteria, rows, out);
    if (rc != PISCES_OK) return rc;
    if (reference_length < 0) return fail(nullptr, PISCES_E_INVALID_ARG, "nbhd_build: negative reference length");
    int64_t n = rows->n;
    if (rows->count) n = *rows->count < 0 ? 0 : std::min<int64_t>(n, *rows->count);
    const nbhd::View v = {rows->recs, rows->cand_index, rows->cands, rows->alleles};
    int64_t* const n_out = out->n_out;
    auto refuse = [&](int32_t code, int64_t which, int64_t row, const std::string& message) {
        for (int c = 0; c < 6; c++) n_out[c] = 0;
        n_out[0] = code;
        n_out[1] = which;
        n_out[2] = row;
        return fail(nullptr, code, message);
    };

    // the rows: what each is, and the eligible ones side by side
    std::vector<uint8_t> bits((size_t)n);
    std::vector<int32_t> e_row, e_pos, e_ref_len, e_alt_len;
    int64_t descending = -1, no_alleles = -1;
    for (int64_t r = 0; r < n; r++) {
        bits[r] = nbhd::row_bits(v, *criteria, r);
        if (descending < 0 && r > 0 && v.recs[r].position < v.recs[r - 1].position) descending = r;
        if (no_alleles < 0 && (bits[r] & nbhd::kNoAlleles)) no_alleles = r;
        if (!(bits[r] & nbhd::kEligible)) continue;
        int32_t ref_len, alt_len;
        nbhd::allele_lengths(v, r, &ref_len, &alt_len);
        e_row.push_back((int32_t)r);
        e_pos.push_back(v.recs[r].position);
        e_ref_len.push_back(ref_len);
        e_alt_len.push_back(alt_len);
    }
    if (descending >= 0) return refuse(PISCES_E_INVALID_ARG, 0, descending, "nbhd_build: the rows are not sorted by position at row " + std::to_string(descending));
    if (no_alleles >= 0)
        return refuse(PISCES_E_INVALID_ARG, 1, no_alleles, "nbhd_build: row " + std::to_string(no_alleles) + " is an insertion, deletion or MNV without a candidate to take its alleles from");

    // the links, the members' passing counts and allele bytes in front of every eligible row, the raw neighbourhoods
    const int64_t n_eligible = (int64_t)e_row.size();
    std::vector<uint8_t> link((size_t)n_eligible);
    std::vector<int64_t> e_bytes((size_t)n_eligible + 1, 0);
    std::vector<int32_t> e_passing((size_t)n_eligible + 1, 0), e_nbhd((size_t)n_eligible, -1), nb_first, nb_end;
    for (int64_t e = 0; e < n_eligible; e++) {
        link[e] = (uint8_t)(nbhd::link_bits(v, e_row.data(), n_eligible, e, criteria->phasing_distance) | ((bits[e_row[e]] & nbhd::kPassing) ? nbhd::kIsPassing : 0));
        const bool member = link[e] & nbhd::kMember;
        e_bytes[e + 1] = e_bytes[e] + (member ? (int64_t)e_ref_len[e] + e_alt_len[e] : 0);
        e_passing[e + 1] = e_passing[e] + (member && (link[e] & nbhd::kIsPassing) ? 1 : 0);
        if (link[e] & nbhd::kHead) nb_first.push_back((int32_t)e);
        if (member) e_nbhd[e] = (int32_t)nb_first.size() - 1;
        if (link[e] & nbhd::kTail) nb_end.push_back((int32_t)e + 1);
    }
    const int64_t n_raw = (int64_t)nb_first.size();

    // which are kept, and what lies in front of each
    std::vector<uint8_t> keep((size_t)n_raw);
    std::vector<int64_t> prefix(4 * (size_t)n_raw + 4, 0);
    for (int64_t nb = 0; nb < n_raw; nb++) {
        const int32_t first = nb_first[nb], end = nb_end[nb];
        const int64_t n_sites = end - first, n_passing = e_passing[end] - e_passing[first];
        keep[nb] = !nbhd::dropped(n_passing, n_sites - n_passing, criteria->min_passing_variants_in_nbhd);
        int64_t look = e_pos[first];
        for (int32_t e = first; e < end; e++) look = std::max<int64_t>(look, (int64_t)e_pos[e] + std::max(e_ref_len[e], e_alt_len[e]));
        const int64_t add[4] = {1, n_sites, e_bytes[end] - e_bytes[first], look - e_pos[first]};
        for (int c = 0; c < 4; c++) prefix[4 * (nb + 1) + c] = prefix[4 * nb + c] + (keep[nb] ? add[c] : 0);
    }
    const int64_t* const total = prefix.data() + 4 * n_raw;
    if (total[2] > 0x7fffffffll || total[3] > 0x7fffffffll) return refuse(PISCES_E_UNSUPPORTED, 0, 0, "nbhd_build: more than 2^31 - 1 allele or reference bytes");
    for (int c = 0; c < 4; c++) n_out[c] = total[c];
    n_out[4] = n_raw;
    n_out[5] = n_eligible;
    if (total[0] > out->nbhd_capacity || total[1] > out->site_capacity || total[2] > out->allele_capacity || total[3] > out->ref_capacity)
        return fail(nullptr, PISCES_E_BUFFER_TOO_SMALL, "nbhd_build: " + std::to_string(total[0]) + " neighbourhoods, " + std::to_string(total[1]) + " sites, " +
                                                            std::to_string(total[2]) + " allele bytes and " + std::to_string(total[3]) + " reference bytes do not fit the capacities");

    // the tables
    if (out->row_class)
        for (int64_t r = 0; r < n; r++)
            if (!(bits[r] & nbhd::kEligible)) out->row_class[r] = (bits[r] & nbhd::kForced) ? PISCES_NBHD_ROW_FORCED : PISCES_NBHD_ROW_INELIGIBLE;
    for (int64_t e = 0; e < n_eligible; e++) {
        const int32_t row = e_row[e];
        if (!(link[e] & nbhd::kMember)) {
            if (out->row_class) out->row_class[row] = PISCES_NBHD_ROW_LONE;
            continue;
        }
        const int32_t nb = e_nbhd[e];
        if (out->row_class) out->row_class[row] = keep[nb] ? PISCES_NBHD_ROW_KEPT : PISCES_NBHD_ROW_DROPPED;
        if (!keep[nb]) continue;
        const int64_t first = nb_first[nb], end = nb_end[nb];
        int64_t group, bytes_in_front;
        const int64_t slot = nbhd::sorted_slot(e_pos.data(), e_ref_len.data(), e_alt_len.data(), first, end, e, &group, &bytes_in_front);
        const int64_t site_base = prefix[4 * nb + 1], byte_base = prefix[4 * nb + 2];
        const int64_t s = site_base + (slot - first);
        const int64_t offset = byte_base + (e_bytes[group] - e_bytes[first]) + bytes_in_front;
        out->sites[s] = PiscesVeadSite{e_pos[e], e_ref_len[e], e_alt_len[e], (int32_t)offset};
        nbhd::copy_alleles(v, row, out->alleles + offset);
        out->site_row[s] = row;
        out->site_original[site_base + (e - first)] = row;
    }
    for (int64_t nb = 0; nb < n_raw; nb++) {
        if (!keep[nb]) continue;
        const int32_t first = nb_first[nb], end = nb_end[nb];
        const int64_t k = prefix[4 * nb], site_begin = prefix[4 * nb + 1], ref_offset = prefix[4 * nb + 3];
        const int32_t n_sites = end - first, n_passing = e_passing[end] - e_passing[first];
        out->neighbourhoods[k] = PiscesVeadNeighborhood{(int32_t)site_begin, (int32_t)site_begin + n_sites};
        const PiscesNbhdInfo info = nbhd::make_info(out->sites, (int32_t)site_begin, (int32_t)site_begin + n_sites, (int32_t)nb, n_passing, n_sites - n_passing, ref_offset);
        out->info[k] = info;
        const vead::Bounds b = {info.first, info.last_with_look_ahead, info.soft_clip_end_before, info.soft_clip_pos_after};
        for (int64_t j = 0; j < info.ref_len; j++) out->ref_bytes[ref_offset + j] = nbhd::reference_byte(reference, reference_length, b, j);
    }
    return PISCES_OK;
    });
}

int32_t pisces_hip_nbhd_build_device(PiscesHip* h, const PiscesNbhdCriteria* criteria, const PiscesVennRows* rows, const PiscesNbhdOut* out, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    const int32_t rc = nbhd_check(h, "nbhd_build_device", criteria, rows, out);
    if (rc != PISCES_OK) return rc;
    nbhddev::Args K;
    std::memset(&K, 0, sizeof(K));
    K.rows = *rows;
    K.criteria = *criteria;
    K.out = *out;
    K.reference = h->ref_len > 0 ? h->d_ref.p : nullptr;
    K.reference_len = h->ref_len;
    const size_t n = (size_t)std::max<int64_t>(rows->n, 1), n_nbhd = n / 2 + 1;
    const unsigned blocks = (unsigned)((n + nbhddev::kBlock - 1) / nbhddev::kBlock), nbhd_blocks = (unsigned)((n_nbhd + nbhddev::kBlock - 1) / nbhddev::kBlock);
    const size_t n_waves = (size_t)blocks * (nbhddev::kBlock / 64);
    K.n_waves = (int32_t)n_waves;
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    // the scratch grows only; an earlier call of this handle may still read what growing gives back (as pisces_hip_venn_consensus_device)
    PiscesHip::NbhdScratch& S = h->nbhd;
    if (n > S.rows || !S.ctrl.p) {
        if (h->foreign_stream_ever) PISCES_HIP_CHECK(h, hipDeviceSynchronize());
        else PISCES_HIP_CHECK(h, hipStreamSynchronize(s));
        PISCES_HIP_CHECK(h, S.bytes.reserve(2 * n + n_nbhd));                // row_bits, e_link, nb_keep
        PISCES_HIP_CHECK(h, S.i32.reserve(n_waves + 6 * n + 1 + 3 * n_nbhd)); // wave_eligible, e_row, e_pos, e_ref_len, e_alt_len, e_nbhd, e_passing, nb_first, nb_end, nb_look
        PISCES_HIP_CHECK(h, S.i64.reserve(4 * n_waves + n + 1 + 4 * n_nbhd)); // wave_eligible_prefix, wave_sum, e_bytes, nb_prefix
        PISCES_HIP_CHECK(h, S.ctrl.reserve(nbhddev::kCtrlWords));
        S.rows = n;
    }
    K.row_bits = S.bytes.p;
    K.e_link = K.row_bits + n;
    K.nb_keep = K.e_link + n;
    K.wave_eligible = S.i32.p;
    K.e_row = K.wave_eligible + n_waves;
    K.e_pos = K.e_row + n;
    K.e_ref_len = K.e_pos + n;
    K.e_alt_len = K.e_ref_len + n;
    K.e_nbhd = K.e_alt_len + n;
    K.e_passing = K.e_nbhd + n;
    K.nb_first = K.e_passing + n + 1;
    K.nb_end = K.nb_first + n_nbhd;
    K.nb_look = K.nb_end + n_nbhd;
    K.wave_eligible_prefix = S.i64.p;
    K.wave_sum = K.wave_eligible_prefix + n_waves;
    K.e_bytes = K.wave_sum + 3 * n_waves;
    K.nb_prefix = K.e_bytes + n + 1;
    K.ctrl = S.ctrl.p;
    PISCES_HIP_CHECK(h, hipMemsetAsync(K.ctrl, 0xff, 2 * sizeof(unsigned long long), s));      // no row descends, none lacks its alleles
    PISCES_HIP_CHECK(h, hipMemsetAsync(K.nb_look, 0x80, n_nbhd * sizeof(int32_t), s));         // below every position
    hipLaunchKernelGGL(nbhddev::nbhd_class_kernel, dim3(blocks), dim3(nbhddev::kBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_scan_rows_kernel, dim3(1), dim3(nbhddev::kScanBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_compact_kernel, dim3(blocks), dim3(nbhddev::kBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_link_kernel, dim3(blocks), dim3(nbhddev::kBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_scan_links_kernel, dim3(1), dim3(nbhddev::kScanBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_index_kernel, dim3(blocks), dim3(nbhddev::kBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_scan_nbhds_kernel, dim3(1), dim3(nbhddev::kScanBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_sites_kernel, dim3(blocks), dim3(nbhddev::kBlock), 0, s, K);
    hipLaunchKernelGGL(nbhddev::nbhd_info_kernel, dim3(nbhd_blocks), dim3(nbhddev::kBlock), 0, s, K);
    if (out->ref_capacity > 0) {
        const unsigned ref_blocks = (unsigned)std::min<int64_t>((out->ref_capacity + nbhddev::kBlock - 1) / nbhddev::kBlock, 4096);
        hipLaunchKernelGGL(nbhddev::nbhd_reference_kernel, dim3(ref_blocks), dim3(nbhddev::kBlock), 0, s, K);
    }
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}
