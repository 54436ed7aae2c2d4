// bisbm_mode_marginals.hip -- mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): one aligned histogram per
// posterior mode, each mode aligned to a reference of its own.  The caller assigns chains to modes (bisbm_marginals_set_modes,
// e.g. from bisbm_partition_modes); a sample is one run of the aligned-sample pipeline of bisbm_align.hip over the counted
// chains, with every mode's reference and into every mode's slice of the histogram.  Anchored modes
// (bisbm_marginals_set_mode_anchors) take the assignment afresh at every sample: the counted chains' VI to one anchor partition
// per mode (partition_distances_rows, the kernels of bisbm_partition.hip), the nearest anchor within the threshold on the host,
// then the same pipeline with the anchors as references.  This unit holds the host side only: the assignment, the references,
// the slices and their part of the C ABI.
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

// Anchored modes, the assignment of one sample: the counted chains (all; under replica exchange those on rung 0 now) get the
// mode of their nearest anchor (ties -> the lowest mode) if it is within the threshold.  Every device entry measures its own
// chains against its copy of the anchors; the decision is taken here from the copied matrix.
int assign_to_anchors(bisbm_engine* h) {
    ModeState& m = h->modes;
    const uint32_t M = m.n_modes, C = h->n_chains;
    std::vector<uint32_t> rung(C, 0);
    if (h->temper.L)
        if (int rc = bisbm_tempering_get(h, rung.data(), nullptr)) return rc;
    m.vi_last.assign((size_t)C * M, std::numeric_limits<double>::quiet_NaN());
    auto measure = [&](bisbm_engine* d, size_t i) {
        const uint32_t first = h->devs.empty() ? 0u : h->dev_first[i];
        std::vector<uint32_t> cold;
        for (uint32_t c = 0; c < d->n_chains; ++c)
            if (rung[first + c] == 0u) cold.push_back(c);
        std::vector<double> vi(cold.size() * M);
        if (int rc = partition_distances_rows(d, cold, d->modes.d_anchor.get(), d->label_stride, M, vi.data())) return rc;
        for (size_t y = 0; y < cold.size(); ++y) std::copy(vi.begin() + y * M, vi.begin() + (y + 1) * M, m.vi_last.begin() + (size_t)(first + cold[y]) * M);
        return (int)BISBM_OK;
    };
    DeviceGuard keep;
    if (int rc = h->devs.empty() ? measure(h, 0) : on_devices(h, measure)) return rc;
    m.pending_unassigned = 0;
    for (uint32_t c = 0; c < C; ++c) {
        m.of_chain[c] = kNone;
        if (rung[c] != 0u) continue;
        const double* v = m.vi_last.data() + (size_t)c * M;
        uint32_t best = 0;
        for (uint32_t g = 1; g < M; ++g)
            if (v[g] < v[best]) best = g;
        if (v[best] <= m.threshold)
            m.of_chain[c] = best;
        else
            m.pending_unassigned += 1;
    }
    ++m.list_serial;  // (the list of counted chains is this sample's)
    return BISBM_OK;
}

// the modes are off again: the histograms, the anchors and the scratch go back
void drop_mode_buffers(bisbm_engine* h, bool off) {
    block_sums_restart(h);  // (block summaries of another assignment are gone with the histograms)
    for (bisbm_engine* d : device_entries(h)) {
        d->modes.slices = 0;
        d->modes.scratch.have_perm = false;
        d->modes.d_counts.reset();
        d->modes.d_anchor.reset();
        if (off) d->modes = ModeState();
    }
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
    std::fill(m.visits.begin(), m.visits.end(), 0);
    m.unassigned = m.samples = 0;
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
            if (m.anchored)
                return fail(h, BISBM_ERR_STATE, "the anchor of mode %u was set for %u + %u blocks, the chains now have %u + %u: set the anchors again", g, r.ka,
                            r.kb, ka, kb);
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
    if (m.anchored)
        if (int rc = assign_to_anchors(h)) return rc;
    AlignPlan plan;
    plan.n_modes = m.n_modes;
    plan.of_chain = m.of_chain.data();
    plan.refs = m.refs.data();
    plan.list_serial = m.list_serial, plan.ref_serial = m.ref_serial;
    if (int rc = block_sums_prepare(h, ka, kb, m.of_chain, plan)) return rc;
    // (device entry i holds the chains dev_first[i] .. of the handle; a plain handle is its own only entry)
    auto sample = [&](bisbm_engine* d, size_t i) { return aligned_sample(d, d->modes.scratch, plan, h->devs.empty() ? 0u : h->dev_first[i], d->modes.d_counts.get()); };
    const int rc = h->devs.empty() ? sample(h, 0) : on_devices(h, sample);
    if (rc) return rc;
    block_sums_commit(h, m.of_chain, plan);
    for (uint32_t c = 0; c < h->n_chains; ++c)
        if (m.of_chain[c] != kNone) {
            m.terms[m.of_chain[c]] += 1;
            if (m.anchored) m.visits[(size_t)c * m.n_modes + m.of_chain[c]] += 1;
        }
    if (m.anchored) {
        m.unassigned += m.pending_unassigned;
        m.samples += 1;
    }
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
    m.anchored = false, m.threshold = 0, m.unassigned = m.samples = 0;
    m.vi_last.clear(), m.visits.clear();
    ++m.list_serial, ++m.ref_serial;
    drop_mode_buffers(h, !n_modes);  // (histograms of another assignment are gone; off: the memory goes back)
    if (!n_modes) m = ModeState();
    return BISBM_OK;
}

int bisbm_marginals_set_mode_anchors(bisbm_handle h, uint32_t n_modes, const uint32_t* anchor_labels, double threshold) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    ModeState& m = h->modes;
    if (!n_modes) {
        if (m.n_modes && h->align.samples)
            return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples counted under the present assignment: bisbm_marginals_reset first");
        if (m.n_modes) {
            drop_mode_buffers(h, true);
            m = ModeState();
        }
        return BISBM_OK;
    }
    if (!anchor_labels) return fail(h, BISBM_ERR_INVALID_ARG, "anchor_labels is NULL");
    if (n_modes == BISBM_MODE_NONE) return fail(h, BISBM_ERR_INVALID_ARG, "n_modes = %u is the value of BISBM_MODE_NONE", n_modes);
    if (!(threshold >= 0.)) return fail(h, BISBM_ERR_INVALID_ARG, "the threshold must be a number >= 0 (+inf: always the nearest anchor), got %g", threshold);
    if (h->align.samples)
        return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples counted under the present assignment: bisbm_marginals_reset first");
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no mode-resolved marginals");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    for (uint32_t g = 0; g < n_modes; ++g)
        if (int rc = check_reference_labels(h, anchor_labels + (size_t)g * h->n, ka, kb)) {
            h->err = "anchor " + std::to_string(g) + ": " + h->err;
            return rc;
        }
    try {
        // a wide handle's labels do not fit the byte rows: it keeps the anchors on the host and is refused at the sample
        const bool bytes = !any_wide(h);
        DeviceGuard keep;
        for (bisbm_engine* d : device_entries(h)) {
            d->modes.slices = 0;
            d->modes.scratch.have_perm = false;
            d->modes.d_counts.reset();
            if (!bytes) continue;
            // (rows padded with zeroes like label rows: the distance kernels load words past n)
            std::vector<uint8_t> rows((size_t)n_modes * d->label_stride, 0);
            for (uint32_t g = 0; g < n_modes; ++g)
                for (uint64_t v = 0; v < h->n; ++v) rows[(size_t)g * d->label_stride + v] = (uint8_t)anchor_labels[(size_t)g * h->n + v];
            HIPCHK(h, hipSetDevice(d->device));
            RESERVE(h, d->modes.d_anchor, rows.size());
            HIPCHK(h, hipMemcpy(d->modes.d_anchor.get(), rows.data(), rows.size(), hipMemcpyHostToDevice));
        }
        block_sums_restart(h);
        m.n_modes = n_modes;
        m.of_chain.assign(h->n_chains, kNone);
        m.refs.assign(n_modes, AlignRef());
        for (uint32_t g = 0; g < n_modes; ++g) {
            AlignRef& r = m.refs[g];
            r.labels.assign(anchor_labels + (size_t)g * h->n, anchor_labels + (size_t)(g + 1) * h->n);
            r.has = true, r.chain = -1, r.ka = ka, r.kb = kb;
        }
        m.terms.assign(n_modes, 0);
        m.anchored = true, m.threshold = threshold;
        m.vi_last.assign((size_t)h->n_chains * n_modes, std::numeric_limits<double>::quiet_NaN());
        m.visits.assign((size_t)h->n_chains * n_modes, 0);
        m.unassigned = m.samples = 0;
        ++m.list_serial, ++m.ref_serial;
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

int bisbm_marginals_get_mode_assignment(bisbm_handle h, double* vi_out, uint64_t* visits_out, uint64_t* unassigned_out, uint64_t* samples_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ModeState& m = h->modes;
    if (!m.anchored) return fail(h, BISBM_ERR_STATE, "no mode anchors are set: bisbm_marginals_set_mode_anchors first");
    if (vi_out) std::copy(m.vi_last.begin(), m.vi_last.end(), vi_out);
    if (visits_out) std::copy(m.visits.begin(), m.visits.end(), visits_out);
    if (unassigned_out) *unassigned_out = m.unassigned;
    if (samples_out) *samples_out = m.samples;
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
    if (h->modes.anchored)
        return fail(h, BISBM_ERR_STATE, "mode anchors are set: every mode is aligned to its anchor (bisbm_marginals_set_mode_anchors sets them)");
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
