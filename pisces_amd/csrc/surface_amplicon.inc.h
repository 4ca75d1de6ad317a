// surface_amplicon.inc.h — part of pisces_hip.hip (included there, inside its extern "C" block; not a translation unit of its own).
// The amplicon-bias filter's entries: AmpliconBiasFilterThreshold (-abfilter) as a switch of the handle, the two adds with an amplicon id
// per read, and IAlleleSource.GetCoverageByAmplicon with the support split.  The ids live in the read store (amplicon_store_ids,
// surface_store.inc.h), the flush's pass is amplicon_launch in call_blocks_enqueue (surface_flush.inc.h).

// what cannot go together with tracking; nullptr: nothing
static const char* amplicon_refusal(const PiscesHip* h)
{
    if (h->cfg.call_mnvs) return "MNV calling is on: SNV candidates come from the read walk, their support by amplicon is not counted";
    if (h->snv_walk) return "the collapse thresholds take SNV candidates from the read walk, their support by amplicon is not counted";
    if (!h->forced.empty()) return "forced alleles are set";
    if (h->read_path != 1) return "PISCES_HIP_READ_PATH=log: observation tuples have no read identity";
    return nullptr;
}

int32_t pisces_hip_set_amplicon_bias_filter(PiscesHip* h, float threshold)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    if (h->stats[2] > 0 || !store_is_empty(h) || h->log_ub > 0 || !h->blocks.empty())
        return fail(h, PISCES_E_STATE, "set_amplicon_bias_filter: reads have been added already");
    const bool on = threshold >= 0.0f;   // (a NaN is null too)
    if (on) {
        const char* why = amplicon_refusal(h);
        if (why) return fail(h, PISCES_E_UNSUPPORTED, std::string("set_amplicon_bias_filter: ") + why);
    }
    h->amp_on = on;
    h->amp_threshold = on ? threshold : -1.0f;
    return PISCES_OK;
    });
}

// the ids of the batch into d_amp_in (from the host or from the device), checked: an id below -1 refuses the batch before anything changes
static int32_t amplicon_take_ids(PiscesHip* h, const char* what, const int32_t* ids, int32_t nr, bool on_device)
{
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    PISCES_HIP_CHECK(h, h->d_amp_in.reserve((size_t)nr + 1));
    PISCES_HIP_CHECK(h, h->d_amp_words.reserve(4));
    int32_t bad = 0;
    if (!on_device) {
        for (int32_t i = 0; i < nr; i++) bad |= ids[i] < -1;
    }
    if (!bad) {
        // (behind whatever still reads the buffer on the stream; the caller's array is free again when this returns)
        PISCES_HIP_CHECK(h, hipMemcpyAsync(h->d_amp_in.p, ids, (size_t)nr * sizeof(int32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        if (on_device) {
            PISCES_HIP_CHECK(h, hipMemsetAsync(h->d_amp_words.p + 1, 0, sizeof(int32_t), h->stream));
            hipLaunchKernelGGL(amplicon_check_ids_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, h->stream, (const int32_t*)h->d_amp_in.p, nr, h->d_amp_words.p + 1);
            PISCES_HIP_CHECK(h, hipGetLastError());
            PISCES_HIP_CHECK(h, hipMemcpyAsync(&bad, h->d_amp_words.p + 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        }
        PISCES_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    }
    if (bad) return fail(h, PISCES_E_INVALID_ARG, std::string(what) + ": an amplicon id below -1 (-1 = no tag)");
    return PISCES_OK;
}

int32_t pisces_hip_add_reads_amplicons(PiscesHip* h, const PiscesReadBatch* batch, const int32_t* amplicon_id)
{
    if (!h) return PISCES_E_INVALID_ARG;
    if (!h->amp_on) return pisces_hip_add_reads(h, batch);   // (the ids are ignored: exactly the plain add)
    {
        const int32_t rc = abi_guard<int32_t>(h, [&]() -> int32_t {
            if (!batch || batch->n_reads < 0 || (batch->n_reads > 0 && !amplicon_id)) return fail(h, PISCES_E_INVALID_ARG, "add_reads_amplicons: null buffer");
            if (batch->n_reads == 0) return PISCES_OK;
            return amplicon_take_ids(h, "add_reads_amplicons", amplicon_id, batch->n_reads, false);
        });
        if (rc) return rc;
    }
    h->amp_pending = batch->n_reads > 0 ? h->d_amp_in.p : nullptr;
    const int32_t rc = pisces_hip_add_reads(h, batch);
    h->amp_pending = nullptr;
    return rc;
}

int32_t pisces_hip_add_device_reads_amplicons(PiscesHip* h, const PiscesReadBatch* device_batch, int64_t n_cigar_ops, int64_t n_bases, const int32_t* device_amplicon_id)
{
    if (!h) return PISCES_E_INVALID_ARG;
    if (!h->amp_on) return pisces_hip_add_device_reads(h, device_batch, n_cigar_ops, n_bases);
    {
        const int32_t rc = abi_guard<int32_t>(h, [&]() -> int32_t {
            if (!device_batch || device_batch->n_reads < 0 || (device_batch->n_reads > 0 && !device_amplicon_id))
                return fail(h, PISCES_E_INVALID_ARG, "add_device_reads_amplicons: null buffer");
            if (device_batch->n_reads == 0) return PISCES_OK;
            return amplicon_take_ids(h, "add_device_reads_amplicons", device_amplicon_id, device_batch->n_reads, true);
        });
        if (rc) return rc;
    }
    h->amp_pending = device_batch->n_reads > 0 ? h->d_amp_in.p : nullptr;
    const int32_t rc = pisces_hip_add_device_reads(h, device_batch, n_cigar_ops, n_bases);
    h->amp_pending = nullptr;
    return rc;
}

// IAlleleSource.GetCoverageByAmplicon(position) for [start_position, start_position + n), with the support split: the histogram half of
// amplicon_tiles_kernel over the held blocks of the range, the slots of every position sorted by id on the way out
int32_t pisces_hip_get_amplicon_counts(PiscesHip* h, int32_t start_position, int32_t n, int32_t* ids, int32_t* coverage, int32_t* support)
{
    return abi_guard<int32_t>(h, [&]() -> int32_t {
    if (!h) return PISCES_E_INVALID_ARG;
    if (n < 0 || (n > 0 && (!ids || !coverage || !support))) return fail(h, PISCES_E_INVALID_ARG, "get_amplicon_counts: null output");
    if (start_position <= 0) return fail(h, PISCES_E_INVALID_ARG, "Position must be greater than 0.");
    if (!h->amp_on) return fail(h, PISCES_E_STATE, "get_amplicon_counts: the handle tracks no amplicon counts (pisces_hip_set_amplicon_bias_filter)");
    for (int64_t i = 0; i < (int64_t)n * kAmpSlots; i++) { ids[i] = -1; coverage[i] = 0; }
    std::memset(support, 0, (size_t)n * 4 * kAmpSlots * sizeof(int32_t));
    if (n == 0) return PISCES_OK;
    PISCES_HIP_CHECK(h, hipSetDevice(h->device));
    std::vector<int32_t> keys;
    for (int32_t k = block_key(h, start_position); k <= block_key(h, start_position + n - 1); k++)
        if (h->blocks.count(k)) keys.push_back(k);
    if (keys.empty()) return PISCES_OK;
    std::vector<PiscesTile> tiles;
    { int32_t rc = bucket_blocks(h, keys, false, tiles); if (rc) return rc; }
    const int32_t n_tiles = (int32_t)tiles.size();
    if (n_tiles == 0) return PISCES_OK;
    const size_t words = (size_t)n_tiles * kTile * kAmpLocusWords;
    PISCES_HIP_CHECK(h, h->d_amp_table.reserve(words));
    const RegularTiles R = {0, h->cfg.block_size, 1, 0};
    { int32_t rc = amplicon_launch(h, "get_amplicon_counts", h->d_tiles.p, R, n_tiles, nullptr, nullptr, h->d_amp_table.p); if (rc) return rc; }
    std::vector<int32_t> host(words);
    PISCES_HIP_CHECK(h, hipMemcpyAsync(host.data(), h->d_amp_table.p, words * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    PISCES_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    static const int kAcgtOfType[4] = {0, 2, 1, 3};   // AlleleType A G C T -> the output's A C G T
    for (int32_t t = 0; t < n_tiles; t++)
        for (int32_t l = 0; l < tiles[(size_t)t].n_loci; l++) {
            const int32_t p = tiles[(size_t)t].start_position + l;
            if (p < start_position || p >= start_position + n) continue;
            const int32_t* row = host.data() + ((size_t)t * kTile + (size_t)l) * kAmpLocusWords;
            int order[kAmpSlots], m = 0;
            for (int s = 0; s < kAmpSlots; s++) if (row[s] != -1) order[m++] = s;
            std::sort(order, order + m, [&](int a, int b) { return row[a] < row[b]; });
            const size_t o = (size_t)(p - start_position);
            for (int j = 0; j < m; j++) {
                const int s = order[j];
                ids[o * kAmpSlots + (size_t)j] = row[s];
                for (int a = 0; a < 4; a++) {
                    const int32_t c = row[kAmpSlots + a * kAmpSlots + s];
                    coverage[o * kAmpSlots + (size_t)j] += c;
                    support[(o * 4 + (size_t)kAcgtOfType[a]) * kAmpSlots + (size_t)j] = c;
                }
            }
        }
    return PISCES_OK;
    });
}
