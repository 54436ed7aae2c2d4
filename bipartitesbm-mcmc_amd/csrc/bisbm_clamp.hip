// bisbm_clamp.hip -- clamped nodes: one mask per handle, a non-zero byte holds the node at its label in every chain (no reference
// counterpart; include/bisbm.h, "Clamped nodes", states what every sampler does with such a node).  This unit keeps the mask: the
// host copy on the handle the caller holds, and on every device entry the device copy with the ascending lists of the open
// nodes of each type.  The kernels that read them are the samplers' own: sweep_kernel and shuffle_philox_clamped_kernel
// (bisbm_kernels.hip), heatbath_kernel (bisbm_heatbath.hip), reshuffle_kernel (bisbm_reshuffle.hip); each is handed the mask
// only while it is not empty (ClampState::mask_or_null), so a handle without a clamp runs what it ran before.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

// the mask (0 / 1 bytes, n_clamped of them set; empty: none) onto one device entry
int clamp_upload(bisbm_engine* e, const std::vector<uint8_t>& mask, uint64_t n_clamped) {
    ClampState& st = e->clamp;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (no kernel of this entry reads the old mask any more)
    if (n_clamped == 0) {
        st = ClampState();
        return constraints_rebuild_open(e, mask);  // (the shuffle's list under block constraints follows the clamp)
    }
    std::vector<uint32_t> open;
    open.reserve((size_t)(e->n - n_clamped));
    uint32_t open_a = 0;
    for (uint64_t v = 0; v < e->n; ++v)
        if (!mask[v]) {
            open.push_back((uint32_t)v);
            open_a += v < e->na ? 1u : 0u;
        }
    RESERVE(e, st.d_mask, (size_t)e->n);
    RESERVE(e, st.d_open, open.size());
    HIPCHK(e, hipMemcpy(st.d_mask.get(), mask.data(), (size_t)e->n, hipMemcpyHostToDevice));
    if (!open.empty()) HIPCHK(e, hipMemcpy(st.d_open.get(), open.data(), sizeof(uint32_t) * open.size(), hipMemcpyHostToDevice));
    st.open_a = open_a, st.open_b = (uint32_t)open.size() - open_a;
    st.n_clamped = n_clamped;
    return constraints_rebuild_open(e, mask);
}

}  // namespace

extern "C" {

int bisbm_clamp_set(bisbm_handle h, const uint8_t* mask) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "clamped nodes are defined in Philox mode: this handle runs BISBM_RNG_MT19937_COMPAT, the mode of parity with the reference, which has no clamp");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "clamped nodes serve byte labels only (at most 256 blocks): merge the blocks down first");
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle have different block counts: a clamp needs one shape for all chains");
    std::vector<uint8_t> m01, old;  // the new mask as 0 / 1 bytes; the one in place, should a device refuse the new one
    uint64_t n_clamped = 0;
    const uint64_t old_n = h->clamp.n_clamped;
    try {
        old = h->clamp.mask;
        if (mask) m01.resize((size_t)h->n);
    } catch (...) {
        return fail(h, BISBM_ERR_STATE, "bisbm_clamp_set: out of host memory");
    }
    for (uint64_t v = 0; mask && v < h->n; ++v) n_clamped += (m01[v] = mask[v] ? 1 : 0);
    if (n_clamped == 0) m01.clear();
    DeviceGuard keep;
    for (bisbm_engine* e : device_entries(h)) {
        int rc = BISBM_OK;
        try {
            rc = clamp_upload(e, m01, n_clamped);
        } catch (...) {
            rc = fail(e, BISBM_ERR_STATE, "bisbm_clamp_set: out of host memory");
        }
        if (rc) {  // nothing changed: this entry and the ones before it take the old mask again
            const std::string msg = e->err;
            for (bisbm_engine* d : device_entries(h)) {
                d->clamp = ClampState();
                (void)clamp_upload(d, old, old_n);
                if (d == e) break;
            }
            h->clamp.mask.swap(old), h->clamp.n_clamped = old_n;
            h->err = msg;
            return rc;
        }
    }
    h->clamp.mask.swap(m01);
    h->clamp.n_clamped = n_clamped;
    return BISBM_OK;
}

int bisbm_clamp_get(bisbm_handle h, uint8_t* mask_out, uint64_t* n_clamped_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (mask_out) {
        if (h->clamp.n_clamped)
            std::memcpy(mask_out, h->clamp.mask.data(), (size_t)h->n);
        else
            std::memset(mask_out, 0, (size_t)h->n);
    }
    if (n_clamped_out) *n_clamped_out = h->clamp.n_clamped;
    return BISBM_OK;
}

}  // extern "C"
