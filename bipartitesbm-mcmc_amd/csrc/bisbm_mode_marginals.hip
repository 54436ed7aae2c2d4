// bisbm_mode_marginals.hip -- mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): one aligned histogram per
// posterior mode, each mode aligned to a reference of its own.  The caller assigns chains to modes (bisbm_marginals_set_modes,
// e.g. from bisbm_partition_modes); a sample is one run of the aligned-sample pipeline of bisbm_align.hip over the counted
// chains, with every mode's reference and into every mode's slice of the histogram.  This unit holds the host side only: the
// assignment, the references, the slices and their part of the C ABI.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kNone = BISBM_MODE_NONE;

int check_mode(bisbm_engine* h, uint32_t mode) {
    if (!h->modes.n_modes) return fail(h, BISBM_ERR_STATE, "no modes are set: bisbm_marginals_set_modes first");
    if (mode >= h->modes.n_modes) return fail(h, BISBM_ERR_INVALID_ARG, "mode %u out of range: %u modes are set", mode, h->modes.n_modes);
    return BISBM_OK;
}

// does every device entry hold histograms of the present assignment and block counts?
bool histograms_fit(bisbm_engine* h, uint32_t ka, uint32_t kb) {
    for (bisbm_engine* d : device_entries(h))
        if (!d->modes.d_counts || d->modes.hist_ka != ka || d->modes.hist_kb != kb || d->modes.slices != h->modes.n_modes) return false;
    return true;
}

}  // namespace

namespace bisbm {

int refuse_while_modes(bisbm_engine* h, const char* call, const char* per_mode_call) {
    if (!h->modes.n_modes) return BISBM_OK;
    return fail(h, BISBM_ERR_STATE, "%s: mode-resolved marginals are set (%u modes, each in the numbering of its own reference): use %s", call,
                h->modes.n_modes, per_mode_call);
}

int mode_reset(bisbm_engine* h) {
    ModeState& m = h->modes;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    const size_t cnt = (size_t)m.n_modes * (size_t)h->n * kmax;
    DeviceGuard keep;
    for (bisbm_engine* d : device_entries(h)) {
        ModeState& s = d->modes;
        HIPCHK(h, hipSetDevice(d->device));
        s.slices = 0;
        RESERVE(h, s.d_counts, cnt);
        HIPCHK(h, hipMemsetAsync(s.d_counts.get(), 0, sizeof(uint32_t) * cnt, d->stream));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        s.slices = m.n_modes, s.hist_ka = ka, s.hist_kb = kb;
        s.scratch.have_perm = false;
    }
    std::fill(m.terms.begin(), m.terms.end(), 0);
    for (AlignRef& r : m.refs)
        if (r.has && r.chain >= 0) r.has = false;  // (a caller's reference stays)
    return BISBM_OK;
}

int mode_accumulate(bisbm_engine* h, uint32_t* device_counts) {
    ModeState& m = h->modes;
    if (device_counts)
        return fail(h, BISBM_ERR_UNSUPPORTED, "mode-resolved marginals accumulate into the library's histograms, one per mode (device_counts must be NULL); bisbm_marginals_get_mode reads them");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (int rc = refuse_wide_labels(h, ka, kb)) return rc;
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no mode-resolved marginals");
    // (histograms of other block counts, after a merge or split, are started afresh, library-chosen references with them)
    if (!histograms_fit(h, ka, kb))
        if (int rc = bisbm_marginals_reset(h)) return rc;
    std::vector<double> S;
    for (uint32_t g = 0; g < m.n_modes; ++g) {
        AlignRef& r = m.refs[g];
        if (r.has && (r.ka != ka || r.kb != kb)) {
            if (r.chain < 0)
                return fail(h, BISBM_ERR_STATE, "the reference partition of mode %u was set for %u + %u blocks, the chains now have %u + %u: set it again", g,
                            r.ka, r.kb, ka, kb);
            r.has = false;
        }
        if (!r.has) {
            if (S.empty()) {
                S.resize(h->n_chains);
                if (int rc = bisbm_entropy(h, S.data())) return rc;
            }
            // (the member chain of the lowest description length; every mode has a member: set_modes)
            if (int rc = pick_reference(h, S, [&](uint32_t c) { return m.of_chain[c] == g; }, ka, kb, r)) return rc;
            ++m.ref_serial;
        }
    }
    AlignPlan plan;
    plan.n_modes = m.n_modes;
    plan.of_chain = m.of_chain.data();
    plan.refs = m.refs.data();
    plan.list_serial = m.list_serial, plan.ref_serial = m.ref_serial;
    // (device entry i holds the chains dev_first[i] .. of the handle; a plain handle is its own only entry)
    auto sample = [&](bisbm_engine* d, size_t i) { return aligned_sample(d, d->modes.scratch, plan, h->devs.empty() ? 0u : h->dev_first[i], d->modes.d_counts.get()); };
    const int rc = h->devs.empty() ? sample(h, 0) : on_devices(h, sample);
    if (rc) return rc;
    for (uint32_t c = 0; c < h->n_chains; ++c)
        if (m.of_chain[c] != kNone) m.terms[m.of_chain[c]] += 1;
    return BISBM_OK;
}

int mode_get_alignment(bisbm_engine* h, uint32_t chain, uint32_t* perm_out, uint64_t* overlap_out) {
    if (h->modes.of_chain[chain] == kNone) return fail(h, BISBM_ERR_STATE, "chain %u is in no mode (BISBM_MODE_NONE): it is not counted", chain);
    uint32_t local = chain;
    bisbm_engine* e = h->devs.empty() ? h : h->devs[dev_of_chain(h, chain, &local)];
    const AlignScratch& s = e->modes.scratch;
    if (!s.have_perm || s.perm_ka != e->ka || s.perm_kb != e->kb || s.list_uploaded != h->modes.list_serial || !e->groups.empty())
        return fail(h, BISBM_ERR_STATE, "chain %u has no aligned sample of its present block counts", chain);
    return read_alignment(h, e, s, s.pos[local], perm_out, overlap_out);
}

}  // namespace bisbm

extern "C" {

int bisbm_marginals_set_modes(bisbm_handle h, uint32_t n_modes, const uint32_t* mode_of_chain) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    ModeState& m = h->modes;
    if (n_modes && !mode_of_chain) return fail(h, BISBM_ERR_INVALID_ARG, "mode_of_chain is NULL");
    if (n_modes == BISBM_MODE_NONE) return fail(h, BISBM_ERR_INVALID_ARG, "n_modes = %u is the value of BISBM_MODE_NONE", n_modes);
    if (n_modes) {
        std::vector<uint32_t> members(n_modes, 0);
        for (uint32_t c = 0; c < h->n_chains; ++c) {
            if (mode_of_chain[c] == kNone) continue;
            if (mode_of_chain[c] >= n_modes)
                return fail(h, BISBM_ERR_INVALID_ARG, "chain %u is given mode %u: modes are 0 .. %u, or BISBM_MODE_NONE", c, mode_of_chain[c], n_modes - 1);
            members[mode_of_chain[c]] += 1;
        }
        for (uint32_t g = 0; g < n_modes; ++g)
            if (!members[g]) return fail(h, BISBM_ERR_INVALID_ARG, "mode %u has no chain", g);
    }
    if (!n_modes && !m.n_modes) return BISBM_OK;
    if (h->align.samples)
        return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples counted under the present assignment: bisbm_marginals_reset first");
    if (n_modes && h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: chains that trade temperatures have no mode of their own (bisbm_tempering_set with L = 0 first)");
    if (n_modes && any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no mode-resolved marginals");
    m.n_modes = n_modes;
    m.of_chain.assign(mode_of_chain, mode_of_chain + (n_modes ? h->n_chains : 0));
    m.refs.assign(n_modes, AlignRef());
    m.terms.assign(n_modes, 0);
    ++m.list_serial, ++m.ref_serial;
    for (bisbm_engine* d : device_entries(h)) {  // (histograms of another assignment are gone; off: the memory goes back)
        d->modes.slices = 0;
        d->modes.scratch.have_perm = false;
        d->modes.d_counts.reset();
        if (!n_modes) d->modes = ModeState();
    }
    if (!n_modes) m = ModeState();
    return BISBM_OK;
}

int bisbm_marginals_get_modes(bisbm_handle h, uint32_t* n_modes, uint32_t* mode_of_chain, int64_t* ref_chain, uint64_t* terms) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ModeState& m = h->modes;
    if (n_modes) *n_modes = m.n_modes;
    if (!m.n_modes) return BISBM_OK;
    if (mode_of_chain) std::copy(m.of_chain.begin(), m.of_chain.end(), mode_of_chain);
    for (uint32_t g = 0; g < m.n_modes; ++g) {
        if (ref_chain) ref_chain[g] = m.refs[g].has ? m.refs[g].chain : -2;
        if (terms) terms[g] = m.terms[g];
    }
    return BISBM_OK;
}

int bisbm_marginals_set_mode_reference(bisbm_handle h, uint32_t mode, const uint32_t* labels) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = check_mode(h, mode)) return rc;
    AlignRef& r = h->modes.refs[mode];
    if (!labels) {
        r.has = false;
        return BISBM_OK;
    }
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (int rc = check_reference_labels(h, labels, ka, kb)) return rc;
    r.labels.assign(labels, labels + h->n);
    r.has = true, r.chain = -1, r.ka = ka, r.kb = kb;
    ++h->modes.ref_serial;
    return BISBM_OK;
}

int bisbm_marginals_get_mode_reference(bisbm_handle h, uint32_t mode, uint32_t* labels_out, int64_t* chain_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = check_mode(h, mode)) return rc;
    const AlignRef& r = h->modes.refs[mode];
    if (!r.has) return fail(h, BISBM_ERR_STATE, "mode %u has no reference partition (none set, and no sample since the last reset)", mode);
    if (labels_out) std::copy(r.labels.begin(), r.labels.end(), labels_out);
    if (chain_out) *chain_out = r.chain;
    return BISBM_OK;
}

int bisbm_marginals_get_mode(bisbm_handle h, uint32_t mode, uint32_t* counts_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!counts_out) return fail(h, BISBM_ERR_INVALID_ARG, "counts_out is NULL");
    if (int rc = check_mode(h, mode)) return rc;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    if (!histograms_fit(h, ka, kb)) return fail(h, BISBM_ERR_STATE, "no mode-resolved histogram of the present block counts yet");
    const size_t cnt = (size_t)h->n * kmax;
    std::vector<uint32_t> part;
    bool first = true;
    DeviceGuard keep;
    for (bisbm_engine* d : device_entries(h)) {  // the devices' slices of the mode, added on the host
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        if (first) {
            HIPCHK(h, hipMemcpy(counts_out, d->modes.d_counts.get() + mode * cnt, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
        } else {
            part.resize(cnt);
            HIPCHK(h, hipMemcpy(part.data(), d->modes.d_counts.get() + mode * cnt, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; ++i) counts_out[i] += part[i];
        }
        first = false;
    }
    return BISBM_OK;
}

int bisbm_marginals_map_mode(bisbm_handle h, uint32_t mode, uint32_t* labels_out, uint32_t* top_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!labels_out) return fail(h, BISBM_ERR_INVALID_ARG, "labels_out is NULL");
    if (int rc = check_mode(h, mode)) return rc;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    if (!h->modes.terms[mode] || !histograms_fit(h, ka, kb))
        return fail(h, BISBM_ERR_STATE, "mode %u has no sample of the present block counts yet", mode);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    bisbm_engine* e = entries[0];
    ModeState& s = e->modes;
    const size_t cnt = (size_t)h->n * kmax;
    DeviceGuard keep;
    HIPCHK(h, hipSetDevice(e->device));
    const uint32_t* counts = s.d_counts.get() + mode * cnt;
    if (entries.size() > 1) {
        // the other devices' slices of the mode are added onto a copy of the first device's
        RESERVE(h, s.d_sum, cnt);
        RESERVE(h, s.d_stage, cnt);
        HIPCHK(h, hipMemcpyAsync(s.d_sum.get(), counts, sizeof(uint32_t) * cnt, hipMemcpyDeviceToDevice, e->stream));
        for (size_t j = 1; j < entries.size(); ++j) {
            HIPCHK(h, hipMemcpyPeerAsync(s.d_stage.get(), e->device, entries[j]->modes.d_counts.get() + mode * cnt, entries[j]->device,
                                         sizeof(uint32_t) * cnt, e->stream));
            HIPCHK(h, launch_counts_add(s.d_sum.get(), s.d_stage.get(), cnt, e->stream));
        }
        counts = s.d_sum.get();
    }
    RESERVE(h, s.d_lab, (size_t)h->n);
    RESERVE(h, s.d_top, (size_t)h->n);
    HIPCHK(h, launch_marginal_map(counts, (uint32_t)h->n, kmax, 0, (uint32_t)h->n, (uint32_t)h->na, ka, s.d_lab.get(), s.d_top.get(), e->stream));
    std::vector<uint16_t> lab((size_t)h->n);
    HIPCHK(h, hipMemcpyAsync(lab.data(), s.d_lab.get(), sizeof(uint16_t) * h->n, hipMemcpyDeviceToHost, e->stream));
    if (top_out) HIPCHK(h, hipMemcpyAsync(top_out, s.d_top.get(), sizeof(uint32_t) * h->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(h, hipStreamSynchronize(e->stream));
    for (uint64_t v = 0; v < h->n; ++v) labels_out[v] = lab[v];
    return BISBM_OK;
}

}  // extern "C"
