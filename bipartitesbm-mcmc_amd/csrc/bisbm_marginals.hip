// bisbm_marginals.hip -- the per-node label histogram over chains and its MAP labels for one engine; pooling
// over the devices of a handle is bisbm_multi.hip.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace bisbm {

// MAP labels from the internal histogram of one engine (no pooling): argmax kernel + copy
int single_marginals_map(bisbm_engine* h, uint32_t* labels_out) {
    if (int rc = shared_shape(h, nullptr, nullptr)) return rc;
    if (!h->counts_fit(h->ka, h->kb)) return fail(h, BISBM_ERR_STATE, "no marginal histogram of the present block counts yet");
    HIPCHK(h, hipSetDevice(h->device));
    DeviceBuf<uint16_t> d_lab;
    RESERVE(h, d_lab, (size_t)h->n);
    std::vector<uint16_t> lab((size_t)h->n);
    HIPCHK(h, launch_marginal_map(h->d_counts, (uint32_t)h->n, h->counts_cols, 0, (uint32_t)h->n, (uint32_t)h->na, h->ka, d_lab.get(), nullptr, h->stream));
    HIPCHK(h, hipMemcpyAsync(lab.data(), d_lab.get(), sizeof(uint16_t) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint64_t v = 0; v < h->n; ++v) labels_out[v] = lab[v];
    return BISBM_OK;
}

int refuse_rungs_over_groups(bisbm_engine* h) {
    // (a group engine knows no rungs: refused wherever the chains are grouped, on any device entry, raw or aligned)
    if (h->temper.L && any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "replica exchange is on and the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no cold-chain histogram");
    return BISBM_OK;
}

}  // namespace bisbm

extern "C" {

int bisbm_marginals_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    h->align.samples = false;
    block_sums_restart(h);  // (the block summaries live and die with the histogram they accompany)
    if (h->align.ref.has && h->align.ref.chain >= 0) h->align.ref.has = false;  // (a caller's reference stays)
    if (h->modes.n_modes) return mode_reset(h);  // (one histogram per mode instead of the pooled one)
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_marginals_reset(d); });
    if (int rc = shared_shape(h, nullptr, nullptr)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const uint32_t kmax = std::max(h->ka, h->kb);
    const size_t cnt = (size_t)std::max<uint64_t>(h->n, h->counts_rows) * kmax;  // (rows past n stay zero: see DevicePool)
    if (h->d_counts && h->counts_kmax < kmax) {
        (void)hipFree(h->d_counts);
        h->d_counts = nullptr;
    }
    if (!h->d_counts) {
        HIPCHK(h, dalloc(&h->d_counts, cnt));
        h->counts_kmax = kmax;
    }
    h->counts_cols = kmax;
    h->counts_ka = h->ka, h->counts_kb = h->kb;
    HIPCHK(h, hipMemsetAsync(h->d_counts, 0, sizeof(uint32_t) * cnt, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

}  // extern "C"

namespace {

int accumulate_plain(bisbm_engine* h, uint32_t* device_counts) {
    if (!h->devs.empty() && device_counts)
        return fail(h, BISBM_ERR_UNSUPPORTED, "a handle over several devices accumulates into its own buffers (device_counts must be NULL); bisbm_marginals_map pools them");
    if (int rc = shared_shape(h, nullptr, nullptr)) return rc;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_marginals_accumulate(d, nullptr); });
    HIPCHK(h, hipSetDevice(h->device));
    if (!device_counts) {
        // (a histogram made before a merge / split changed the block counts holds another numbering: start afresh)
        if (!h->counts_fit(h->ka, h->kb)) {
            int rc = bisbm_marginals_reset(h);
            if (rc) return rc;
        }
        device_counts = h->d_counts;
    }
    if (!h->groups.empty())  // groups that have come to one shape again: every group adds its chains to the same histogram
        return each_group(h, [&](bisbm_engine* g) { return bisbm_marginals_accumulate(g, device_counts); });
    MarginalParams mp{};
    mp.n = (uint32_t)h->n;
    mp.na = (uint32_t)h->na;
    mp.ka = h->ka;
    mp.kmax = std::max(h->ka, h->kb);
    mp.n_chains = h->n_chains;
    mp.labels = h->d_labels;
    mp.label_stride = h->label_stride;
    mp.wide = h->wide ? 1u : 0u;
    mp.counts = device_counts;
    mp.rung = h->temper.L ? h->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    HIPCHK(h, launch_marginals(mp, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_marginals_accumulate(bisbm_handle h, uint32_t* device_counts) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (h->blocks.what && !h->modes.n_modes && h->align.mode != BISBM_ALIGN_REFERENCE)
        return fail(h, BISBM_ERR_STATE, "block sums are on and this sample is not aligned: raw labels of several chains share no numbering (bisbm_marginals_set_alignment with BISBM_ALIGN_REFERENCE, or modes, first)");
    const int rc = h->modes.n_modes ? mode_accumulate(h, device_counts) : h->align.mode == BISBM_ALIGN_REFERENCE ? align_accumulate(h, device_counts) : accumulate_plain(h, device_counts);
    if (rc == BISBM_OK && !device_counts) h->align.samples = true;
    return rc;
}

int bisbm_marginals_get(bisbm_handle h, uint32_t* counts_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!counts_out) return fail(h, BISBM_ERR_INVALID_ARG, "counts_out is NULL");
    if (int rc = refuse_while_modes(h, "bisbm_marginals_get", "bisbm_marginals_get_mode")) return rc;
    if (!h->devs.empty()) return multi_marginals_get(h, counts_out);
    if (int rc = shared_shape(h, nullptr, nullptr)) return rc;
    if (!h->d_counts) return fail(h, BISBM_ERR_STATE, "no internal marginal buffer yet");
    if (!h->counts_fit(h->ka, h->kb))
        return fail(h, BISBM_ERR_STATE, "the block counts changed since the histogram was made (%u + %u then, %u + %u now)", h->counts_ka, h->counts_kb,
                    h->ka, h->kb);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(counts_out, h->d_counts, sizeof(uint32_t) * (size_t)h->n * std::max(h->ka, h->kb), hipMemcpyDeviceToHost));
    return BISBM_OK;
}

int bisbm_marginals_map(bisbm_handle h, uint32_t* labels_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!labels_out) return fail(h, BISBM_ERR_INVALID_ARG, "labels_out is NULL");
    if (int rc = refuse_while_modes(h, "bisbm_marginals_map", "bisbm_marginals_map_mode")) return rc;
    return h->devs.empty() ? single_marginals_map(h, labels_out) : multi_marginals_map(h, labels_out);
}

}  // extern "C"
