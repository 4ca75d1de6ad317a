// surface_vead.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// Scylla's read pass: the states of one read (vead.h), the bounds of a neighbourhood, and the vead groups of every neighbourhood over a
// host batch and over reads in device memory (vead_kernels.hip.h).  Entries without a handle leave their message where a failed
// pisces_hip_create leaves its own: pisces_hip_last_error(NULL).

static int32_t vead_check_options(PiscesHip* h, const char* what, const PiscesVeadOptions* opts)
{
    if (!opts) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null options");
    if (opts->min_base_call_quality < 0 || opts->min_base_call_quality > 255)
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": min_base_call_quality " + std::to_string(opts->min_base_call_quality) + " is outside [0, 255]");
    return PISCES_OK;
}

static int32_t vead_check_sites(PiscesHip* h, const char* what, const PiscesVeadSite* sites, int32_t n_sites, const uint8_t* alleles, int64_t n_allele_bytes)
{
    if (n_sites < 0 || n_allele_bytes < 0) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": negative size");
    if (n_sites > 0 && (!sites || !alleles)) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null sites or allele bytes");
    for (int32_t i = 0; i < n_sites; i++) {
        const PiscesVeadSite& s = sites[i];
        if (s.ref_len < 1 || s.alt_len < 1)
            return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": site " + std::to_string(i) + " has a ref_len or alt_len below 1");
        if (s.allele_offset < 0 || (int64_t)s.allele_offset + s.ref_len + s.alt_len > n_allele_bytes)
            return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": site " + std::to_string(i) + " has its allele bytes outside the allele array");
    }
    return PISCES_OK;
}

static int32_t vead_check_neighbourhoods(PiscesHip* h, const char* what, int32_t n_sites, const PiscesVeadNeighborhood* nb, int32_t n)
{
    if (n < 0) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": negative neighbourhood count");
    if (n > 0 && !nb) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null neighbourhoods");
    for (int32_t i = 0; i < n; i++) {
        if (nb[i].site_begin < 0 || nb[i].site_end > n_sites || nb[i].site_begin > nb[i].site_end)
            return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": neighbourhood " + std::to_string(i) + " lies outside the site list");
        if (nb[i].site_begin == nb[i].site_end)
            return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": neighbourhood " + std::to_string(i) + " is empty");
        if (nb[i].site_end - nb[i].site_begin > PISCES_VEAD_MAX_SITES)
            return fail(h, PISCES_E_UNSUPPORTED, std::string(what) + ": neighbourhood " + std::to_string(i) + " has " + std::to_string(nb[i].site_end - nb[i].site_begin) +
                                                     " sites, more than PISCES_VEAD_MAX_SITES (" + std::to_string(PISCES_VEAD_MAX_SITES) + ")");
    }
    return PISCES_OK;
}

static int32_t vead_check_out(PiscesHip* h, const char* what, const PiscesVeadOut* out, int32_t n_nbhd)
{
    if (!out) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null out");
    if (!out->n_out) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": null n_out");
    if (out->group_capacity < 0 || out->state_capacity < 0) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": negative capacity");
    if ((out->group_capacity > 0 && !out->groups) || (out->state_capacity > 0 && !out->states) || (n_nbhd > 0 && !out->info))
        return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": a capacity above 0 with a null output array");
    return PISCES_OK;
}

int32_t pisces_hip_vead_default_options(PiscesVeadOptions* opts)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    if (!opts) return fail(nullptr, PISCES_E_INVALID_ARG, "vead_default_options: null options");
    opts->min_base_call_quality = 20;         // BamFilterParameters.MinimumBaseCallQuality
    opts->min_number_variants_in_read = 1;    // BamFilterParameters.MinNumberVariantsInRead
    return PISCES_OK;
    });
}

int32_t pisces_hip_vead_site_states(const PiscesVeadOptions* opts, int32_t position, const uint8_t* cigar_op, const uint32_t* cigar_len, int32_t n_cigar,
                                    const uint8_t* bases, const uint8_t* quals, int32_t n_bases, const PiscesVeadSite* sites, int32_t n_sites,
                                    const uint8_t* alleles, int64_t n_allele_bytes, uint8_t* states, int32_t* n_in_range)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    int32_t rc = vead_check_options(nullptr, "vead_site_states", opts);
    if (rc == PISCES_OK) rc = vead_check_sites(nullptr, "vead_site_states", sites, n_sites, alleles, n_allele_bytes);
    if (rc != PISCES_OK) return rc;
    if (n_cigar < 0 || n_bases < 0 || (n_cigar > 0 && (!cigar_op || !cigar_len)) || (n_bases > 0 && (!bases || !quals)) || (n_sites > 0 && !states))
        return fail(nullptr, PISCES_E_INVALID_ARG, "vead_site_states: a null array or a negative size");
    const vead::ReadView r = {position, cigar_op, cigar_len, n_cigar, bases, quals, n_bases};
    const int32_t found = vead::read_states(r, opts->min_base_call_quality, sites, n_sites, alleles, states);
    if (n_in_range) *n_in_range = found;
    return PISCES_OK;
    });
}

int32_t pisces_hip_vead_neighborhood_info(const PiscesVeadSite* sites, int32_t n_sites, PiscesVeadNeighborhoodInfo* info)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    if (!sites || !info) return fail(nullptr, PISCES_E_INVALID_ARG, "vead_neighborhood_info: null sites or info");
    if (n_sites < 1) return fail(nullptr, PISCES_E_INVALID_ARG, "vead_neighborhood_info: the neighbourhood is empty");
    for (int32_t i = 0; i < n_sites; i++)
        if (sites[i].ref_len < 1 || sites[i].alt_len < 1)
            return fail(nullptr, PISCES_E_INVALID_ARG, "vead_neighborhood_info: site " + std::to_string(i) + " has a ref_len or alt_len below 1");
    const vead::Bounds b = vead::bounds(sites, 0, n_sites);
    std::memset(info, 0, sizeof(*info));
    info->first = b.first;
    info->last_with_look_ahead = b.last_with_look_ahead;
    info->soft_clip_end_before = b.soft_clip_end_before;
    info->soft_clip_pos_after = b.soft_clip_pos_after;
    return PISCES_OK;
    });
}

int32_t pisces_hip_vead_groups(const PiscesVeadOptions* opts, const PiscesReadBatch* batch, const PiscesVeadSite* sites, int32_t n_sites,
                               const uint8_t* alleles, int64_t n_allele_bytes, const PiscesVeadNeighborhood* nbhd, int32_t n_nbhd, const PiscesVeadOut* out)
{
    return abi_guard<int32_t>((PiscesHip*)nullptr, [&]() -> int32_t {
    const char* what = "vead_groups";
    int32_t rc = vead_check_options(nullptr, what, opts);
    if (rc == PISCES_OK) rc = vead_check_sites(nullptr, what, sites, n_sites, alleles, n_allele_bytes);
    if (rc == PISCES_OK) rc = vead_check_neighbourhoods(nullptr, what, n_sites, nbhd, n_nbhd);
    if (rc == PISCES_OK) rc = vead_check_out(nullptr, what, out, n_nbhd);
    if (rc != PISCES_OK) return rc;
    if (!batch || batch->n_reads < 0) return fail(nullptr, PISCES_E_INVALID_ARG, "vead_groups: null batch or a negative read count");
    const int32_t nr = batch->n_reads;
    if (nr > 0 && (!batch->position || !batch->cigar_offset || !batch->cigar_op || !batch->cigar_len || !batch->seq_offset || !batch->bases || !batch->quals))
        return fail(nullptr, PISCES_E_INVALID_ARG, "vead_groups: a null array in the batch");
    for (int32_t r = 0; r < nr; r++)
        if (batch->cigar_offset[r + 1] < batch->cigar_offset[r] || batch->seq_offset[r + 1] < batch->seq_offset[r])
            return fail(nullptr, PISCES_E_INVALID_ARG, "vead_groups: the offsets of read " + std::to_string(r) + " descend");
    for (int32_t r = 1; r < nr; r++)
        if (batch->position[r] < batch->position[r - 1]) {
            out->n_out[0] = PISCES_E_INVALID_ARG;
            out->n_out[1] = 0;
            out->n_out[2] = r;
            return fail(nullptr, PISCES_E_INVALID_ARG, "vead_groups: the reads are not sorted by position at read " + std::to_string(r));
        }
    std::vector<PiscesVeadGroup> groups;
    std::vector<uint8_t> states;
    std::vector<uint8_t> st((size_t)PISCES_VEAD_MAX_SITES);
    for (int32_t n = 0; n < n_nbhd; n++) {
        const int32_t s0 = nbhd[n].site_begin, ns = nbhd[n].site_end - s0;
        const vead::Bounds b = vead::bounds(sites, s0, nbhd[n].site_end);
        PiscesVeadNeighborhoodInfo info;
        std::memset(&info, 0, sizeof(info));
        info.first = b.first;
        info.last_with_look_ahead = b.last_with_look_ahead;
        info.soft_clip_end_before = b.soft_clip_end_before;
        info.soft_clip_pos_after = b.soft_clip_pos_after;
        info.group_begin = (int32_t)groups.size();
        std::unordered_map<std::string, int32_t> by_key;   // the reference's Dictionary<string, VeadGroup>
        for (int32_t r = 0; r < nr; r++) {                  // VeadGroupSource.GetVeadGroups' loop over the alignments
            const int32_t c0 = batch->cigar_offset[r], nc = batch->cigar_offset[r + 1] - c0, q0 = batch->seq_offset[r];
            const int32_t pos = batch->position[r];
            int64_t end = vead::end_position(pos, batch->cigar_op + c0, batch->cigar_len + c0, nc);
            if (end > 0x7FFFFFFFll) end = 0x7FFFFFFFll;
            const bool starts_s = nc > 0 && batch->cigar_op[c0] == 'S', ends_s = nc > 0 && batch->cigar_op[c0 + nc - 1] == 'S';
            bool is_clipped;
            const vead::Verdict verdict = vead::scan_read(pos, end, starts_s, ends_s, b, &is_clipped);
            if (is_clipped) info.n_clipped_reads++;
            if (verdict == vead::kSkip) continue;
            if (verdict == vead::kPast) break;
            info.n_reads_used++;
            const vead::ReadView rv = {pos, batch->cigar_op + c0, batch->cigar_len + c0, nc, batch->bases + q0, batch->quals + q0, batch->seq_offset[r + 1] - q0};
            const int32_t found = vead::read_states(rv, opts->min_base_call_quality, sites + s0, ns, alleles, st.data());
            if (found < opts->min_number_variants_in_read) continue;
            const std::string key((const char*)st.data(), (size_t)ns);
            auto it = by_key.find(key);
            if (it == by_key.end()) {
                by_key.emplace(key, (int32_t)groups.size());
                groups.push_back({n, r, 1, 0, (int64_t)states.size()});
                states.insert(states.end(), st.begin(), st.begin() + ns);
            } else {
                groups[(size_t)it->second].n_veads++;
            }
        }
        info.n_groups = (int32_t)groups.size() - info.group_begin;
        out->info[n] = info;
    }
    out->n_out[0] = (int64_t)groups.size();
    out->n_out[1] = (int64_t)states.size();
    out->n_out[2] = 0;
    if ((int64_t)groups.size() > out->group_capacity || (int64_t)states.size() > out->state_capacity)
        return fail(nullptr, PISCES_E_BUFFER_TOO_SMALL, "vead_groups: " + std::to_string(groups.size()) + " groups and " + std::to_string(states.size()) +
                                                            " state bytes do not fit the capacities");
    if (!groups.empty()) std::memcpy(out->groups, groups.data(), groups.size() * sizeof(PiscesVeadGroup));
    if (!states.empty()) std::memcpy(out->states, states.data(), states.size());
    return PISCES_OK;
    });
}

int32_t pisces_hip_vead_groups_device(PiscesHip* h, const PiscesVeadOptions* opts, const PiscesReadBatch* device_batch, int64_t n_cigar_ops, int64_t n_bases,
                                      const PiscesVeadSite* sites, int32_t n_sites, const uint8_t* alleles, int64_t n_allele_bytes,
                                      const PiscesVeadNeighborhood* nbhd, int32_t n_nbhd, const PiscesVeadOut* out, void* stream)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    const char* what = "vead_groups_device";
    int32_t rc = vead_check_options(h, what, opts);
    if (rc == PISCES_OK) rc = vead_check_sites(h, what, sites, n_sites, alleles, n_allele_bytes);
    if (rc == PISCES_OK) rc = vead_check_neighbourhoods(h, what, n_sites, nbhd, n_nbhd);
    if (rc == PISCES_OK) rc = vead_check_out(h, what, out, n_nbhd);
    if (rc != PISCES_OK) return rc;
    (void)n_cigar_ops;
    (void)n_bases;
    veaddev::Args K;
    std::memset(&K, 0, sizeof(K));
    if (device_batch) {
        if (device_batch->n_reads < 0) return fail(h, PISCES_E_INVALID_ARG, "vead_groups_device: a negative size");
        if (device_batch->n_reads > 0 && (!device_batch->position || !device_batch->cigar_offset || !device_batch->cigar_op || !device_batch->cigar_len ||
                                          !device_batch->seq_offset || !device_batch->bases || !device_batch->quals))
            return fail(h, PISCES_E_INVALID_ARG, "vead_groups_device: a null array in the device batch");
        K.position = device_batch->position;
        K.cigar_offset = device_batch->cigar_offset;
        K.cigar_op = device_batch->cigar_op;
        K.cigar_len = device_batch->cigar_len;
        K.seq_offset = device_batch->seq_offset;
        K.bases = device_batch->bases;
        K.quals = device_batch->quals;
        K.n_reads = device_batch->n_reads;
    } else {
        auto& B = h->bam;
        if (!B.valid) return fail(h, PISCES_E_STATE, "vead_groups_device: no decoded batch (pisces_hip_bam_decode first, or pass a device batch)");
        if (B.moved) return fail(h, PISCES_E_STATE, "vead_groups_device: the decoded batch has been added to the read store (call before pisces_hip_add_decoded_reads)");
        K.position = B.position.p;
        K.cigar_offset = B.cigar_offset.p;
        K.cigar_op = B.cigar_op.p;
        K.cigar_len = B.cigar_len.p;
        K.seq_offset = B.seq_offset.p;
        K.bases = B.bases.p + kSegmentPad;
        K.quals = B.quals.p + kSegmentPad;
        K.n_reads = (int32_t)B.n_reads;
    }
    if (K.n_reads >= veaddev::kNoPair) return fail(h, PISCES_E_UNSUPPORTED, "vead_groups_device: more reads than one call holds");
    K.min_q = opts->min_base_call_quality;
    K.min_sites = opts->min_number_variants_in_read;
    K.n_nbhd = n_nbhd;
    K.out = *out;
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (s != h->stream) h->foreign_stream_used = h->foreign_stream_ever = true;
    auto& V = h->vead;
    // the scratch grows only; an earlier call of this handle may still read what growing gives back (as pisces_hip_venn_consensus_device)
    auto quiet = [&]() -> hipError_t { return h->foreign_stream_ever ? hipDeviceSynchronize() : hipStreamSynchronize(s); };
    const size_t nr = (size_t)K.n_reads, nn = (size_t)n_nbhd;
    if (nr > V.end.cap || nr > V.clip.cap || 2 * nn > V.range.cap || 2 * nn > V.counts.cap || !V.ctrl.p ||
        (size_t)n_sites > V.sites.cap || (size_t)n_allele_bytes > V.alleles.cap || nn > V.nbhd.cap || nn > V.bounds.cap || nn > V.plan.cap) {
        PISCES_HIP_CHECK(h, quiet());
        PISCES_HIP_CHECK(h, V.end.reserve(nr + 1));
        PISCES_HIP_CHECK(h, V.clip.reserve(nr + 1));
        PISCES_HIP_CHECK(h, V.range.reserve(2 * nn + 2));
        PISCES_HIP_CHECK(h, V.counts.reserve(2 * nn + 2));
        PISCES_HIP_CHECK(h, V.ctrl.reserve(2));
        PISCES_HIP_CHECK(h, V.sites.reserve((size_t)n_sites + 1));
        PISCES_HIP_CHECK(h, V.alleles.reserve((size_t)n_allele_bytes + 1));
        PISCES_HIP_CHECK(h, V.nbhd.reserve(nn + 1));
        PISCES_HIP_CHECK(h, V.bounds.reserve(nn + 1));
        PISCES_HIP_CHECK(h, V.plan.reserve(nn + 1));
    }
    std::vector<vead::Bounds> bounds(nn);
    for (size_t n = 0; n < nn; n++) bounds[n] = vead::bounds(sites, nbhd[n].site_begin, nbhd[n].site_end);
    if (n_sites) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.sites.p, sites, (size_t)n_sites * sizeof(PiscesVeadSite), hipMemcpyHostToDevice, s));
    if (n_allele_bytes) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.alleles.p, alleles, (size_t)n_allele_bytes, hipMemcpyHostToDevice, s));
    if (nn) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.nbhd.p, nbhd, nn * sizeof(PiscesVeadNeighborhood), hipMemcpyHostToDevice, s));
    if (nn) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.bounds.p, bounds.data(), nn * sizeof(vead::Bounds), hipMemcpyHostToDevice, s));
    PISCES_HIP_CHECK(h, hipMemsetAsync(V.ctrl.p, 0xff, sizeof(unsigned long long), s));
    PISCES_HIP_CHECK(h, hipMemsetAsync(V.ctrl.p + 1, 0, sizeof(unsigned long long), s));
    if (nn) PISCES_HIP_CHECK(h, hipMemsetAsync(V.counts.p, 0, 2 * nn * sizeof(int32_t), s));
    K.sites = V.sites.p;
    K.alleles = V.alleles.p;
    K.nbhd = V.nbhd.p;
    K.bounds = V.bounds.p;
    K.plan = V.plan.p;
    K.end = V.end.p;
    K.clip = V.clip.p;
    K.range = V.range.p;
    K.counts = V.counts.p;
    K.ctrl = V.ctrl.p;
    if (nr) hipLaunchKernelGGL(veaddev::vead_spans_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, s, K);
    if (nn) hipLaunchKernelGGL(veaddev::vead_ranges_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, K);
    PISCES_HIP_CHECK(h, hipGetLastError());
    // the one wait of the call: the ranges size the scratch, the verdict becomes a status
    std::vector<int32_t> range(2 * nn + 1);
    unsigned long long first_bad = ~0ull;
    if (nn) PISCES_HIP_CHECK(h, hipMemcpyAsync(range.data(), V.range.p, 2 * nn * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PISCES_HIP_CHECK(h, hipMemcpyAsync(&first_bad, V.ctrl.p, sizeof(first_bad), hipMemcpyDeviceToHost, s));
    PISCES_HIP_CHECK(h, hipStreamSynchronize(s));
    if (first_bad != ~0ull) {
        const int64_t triple[3] = {PISCES_E_INVALID_ARG, 0, (int64_t)first_bad};
        PISCES_HIP_CHECK(h, hipMemcpyAsync(out->n_out, triple, sizeof(triple), hipMemcpyDefault, s));
        PISCES_HIP_CHECK(h, hipStreamSynchronize(s));
        return fail(h, PISCES_E_INVALID_ARG, "vead_groups_device: the reads are not sorted by position at read " + std::to_string(first_bad));
    }
    std::vector<veaddev::Plan> plan(nn);
    std::vector<int2> work;
    int64_t pairs = 0, key_words = 0, slots = 0;
    for (size_t n = 0; n < nn; n++) {
        veaddev::Plan& P = plan[n];
        const int32_t lo = range[2 * n], hi = range[2 * n + 1];
        P.lo = lo;
        P.hi = hi;
        P.n_pairs = std::min<int32_t>(hi + 1, K.n_reads) - lo;   // the read the scan stops at is still clip-tested
        P.words = vead::key_words(nbhd[n].site_end - nbhd[n].site_begin);
        P.pair_base = pairs;
        P.key_base = key_words;
        P.table_base = slots;
        uint32_t t = 0;
        if (P.n_pairs > 0) { t = 2; while ((int64_t)t < 2 * (int64_t)P.n_pairs) t <<= 1; }
        P.table_mask = t ? t - 1 : 0;
        P.work_base = (int32_t)work.size();
        for (int32_t k = 0; k < P.n_pairs; k += 64) work.push_back(make_int2((int32_t)n, k));
        pairs += P.n_pairs;
        key_words += (int64_t)P.n_pairs * P.words;
        slots += t;
    }
    if (pairs >= veaddev::kNoPair || slots >= 0x7FFFFFFFll || work.size() >= 0x7FFFFFFFull)
        return fail(h, PISCES_E_UNSUPPORTED, "vead_groups_device: " + std::to_string(pairs) + " (neighbourhood, read) pairs are more than one call holds");
    K.n_pairs = pairs;
    K.n_slots = slots;
    K.n_work = (int32_t)work.size();
    if (work.size() > V.work.cap || (size_t)key_words > V.keys.cap || (size_t)pairs > V.is_vead.cap || (size_t)slots > V.table.cap ||
        (size_t)slots > V.slot_count.cap || (size_t)pairs > V.pair_count.cap || 2 * (work.size() + 1) > V.prefix.cap || work.size() > V.work_groups.cap) {
        PISCES_HIP_CHECK(h, quiet());
        PISCES_HIP_CHECK(h, V.work.reserve(work.size() + 1));
        PISCES_HIP_CHECK(h, V.keys.reserve((size_t)key_words + 1));
        PISCES_HIP_CHECK(h, V.is_vead.reserve((size_t)pairs + 1));
        PISCES_HIP_CHECK(h, V.table.reserve((size_t)slots + 1));
        PISCES_HIP_CHECK(h, V.slot_count.reserve((size_t)slots + 1));
        PISCES_HIP_CHECK(h, V.pair_count.reserve((size_t)pairs + 1));
        PISCES_HIP_CHECK(h, V.prefix.reserve(2 * (work.size() + 1)));
        PISCES_HIP_CHECK(h, V.work_groups.reserve(work.size() + 1));
    }
    K.work = V.work.p;
    K.keys = V.keys.p;
    K.is_vead = V.is_vead.p;
    K.table = V.table.p;
    K.slot_count = V.slot_count.p;
    K.pair_count = V.pair_count.p;
    K.prefix = V.prefix.p;
    K.work_groups = V.work_groups.p;
    if (nn) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.plan.p, plan.data(), nn * sizeof(veaddev::Plan), hipMemcpyHostToDevice, s));
    if (!work.empty()) PISCES_HIP_CHECK(h, hipMemcpyAsync(V.work.p, work.data(), work.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    if (slots) PISCES_HIP_CHECK(h, hipMemsetAsync(V.table.p, 0x7f, (size_t)slots * sizeof(int32_t), s));
    if (slots) PISCES_HIP_CHECK(h, hipMemsetAsync(V.slot_count.p, 0, (size_t)slots * sizeof(int32_t), s));
    if (pairs) PISCES_HIP_CHECK(h, hipMemsetAsync(V.pair_count.p, 0, (size_t)pairs * sizeof(int32_t), s));
    if (K.n_work) {
        hipLaunchKernelGGL(veaddev::vead_states_kernel, dim3((unsigned)K.n_work), dim3(64), 0, s, K);
        hipLaunchKernelGGL(veaddev::vead_group_kernel, dim3((unsigned)K.n_work), dim3(64), 0, s, K);
        hipLaunchKernelGGL(veaddev::vead_mark_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, K);
        hipLaunchKernelGGL(veaddev::vead_count_kernel, dim3((unsigned)K.n_work), dim3(64), 0, s, K);
    }
    hipLaunchKernelGGL(veaddev::vead_scan_kernel, dim3(1), dim3(veaddev::kScanBlock), 0, s, K);
    if (K.n_work) hipLaunchKernelGGL(veaddev::vead_emit_kernel, dim3((unsigned)K.n_work), dim3(64), 0, s, K);
    if (nn) hipLaunchKernelGGL(veaddev::vead_info_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, K);
    PISCES_HIP_CHECK(h, hipGetLastError());
    return PISCES_OK;
    });
}
