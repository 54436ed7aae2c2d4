// bisbm_constraints.hip -- block constraints: a class byte per node and a table of allowed blocks per class; node v may sit in
// block s iff its class allows s and s is of v's type (no reference counterpart; include/bisbm.h, "Block constraints", states
// what every sampler does with them).  This unit keeps the state: the host copies, and on every device entry the class bytes, the
// bit table and the shuffle's list of the open nodes by (type, class).  The kernels that read them are the samplers' own:
// sweep_kernel and shuffle_philox_constrained_kernel (bisbm_kernels.hip), heatbath_kernel (bisbm_heatbath.hip), reshuffle_kernel
// (bisbm_reshuffle.hip); each is handed the pointers only while constraints are set (ConstraintState::bits_or_null), so a handle
// without constraints runs what it ran before.  A new set of constraints is staged and validated on every device entry first --
// constraints_check_kernel reports the first label the table does not allow -- and put in place only when every entry took it.
#include "bisbm_engine.hpp"

#include <algorithm>

using namespace bisbm;

namespace bisbm {

namespace {

// the lowest chain * n + node whose label its class does not allow (first: ~0)
__global__ void constraints_check_kernel(const uint8_t* labels, size_t label_stride, uint32_t n, uint32_t n_chains, const uint8_t* cls,
                                         const uint32_t* bits, unsigned long long* first) {
    const uint32_t chain = blockIdx.y;
    if (chain >= n_chains) return;
    const uint8_t* lab = labels + (size_t)chain * label_stride;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        if (!cn_allows(bits, cls[v], lab[v])) atomicMin(first, (unsigned long long)chain * n + v);
}

// the open nodes under `clamp_mask` (empty: all) sorted by (type, class, id), with the segments of equal (type, class)
int build_open(bisbm_engine* e, ConstraintState& st, const std::vector<uint8_t>& clamp_mask) {
    std::vector<uint32_t> open, seg, key;
    open.reserve((size_t)e->n);
    for (uint64_t v = 0; v < e->n; ++v)
        if (clamp_mask.empty() || !clamp_mask[v]) open.push_back((uint32_t)v);
    auto key_of = [&](uint32_t v) { return ((v < e->na ? 0u : 1u) << 8) | (uint32_t)st.cls[v]; };
    std::stable_sort(open.begin(), open.end(), [&](uint32_t x, uint32_t y) { return key_of(x) < key_of(y); });
    for (size_t i = 0; i < open.size(); ++i)
        if (i == 0 || key_of(open[i]) != key_of(open[i - 1])) seg.push_back((uint32_t)i), key.push_back(key_of(open[i]));
    st.n_segs = (uint32_t)key.size();
    seg.push_back((uint32_t)open.size());
    RESERVE(e, st.d_open, std::max<size_t>(open.size(), 1));
    RESERVE(e, st.d_seg, seg.size());
    RESERVE(e, st.d_seg_key, std::max<size_t>(key.size(), 1));
    if (!open.empty()) HIPCHK(e, hipMemcpy(st.d_open.get(), open.data(), sizeof(uint32_t) * open.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(st.d_seg.get(), seg.data(), sizeof(uint32_t) * seg.size(), hipMemcpyHostToDevice));
    if (!key.empty()) HIPCHK(e, hipMemcpy(st.d_seg_key.get(), key.data(), sizeof(uint32_t) * key.size(), hipMemcpyHostToDevice));
    return BISBM_OK;
}

// one device entry's new state into `st`, checked against the labels its chains hold now; the entry itself is not touched
int stage(bisbm_engine* e, ConstraintState& st, uint32_t n_classes, const uint8_t* cls, const uint8_t* allowed,
          const std::vector<uint32_t>& bits, const std::vector<uint8_t>& clamp_mask) {
    HIPCHK(e, hipSetDevice(e->device));
    st.n_classes = n_classes;
    st.cls.assign(cls, cls + e->n);
    st.allowed.assign(allowed, allowed + (size_t)n_classes * e->K);
    st.bits = bits;
    DeviceBuf<unsigned long long> d_first;
    RESERVE(e, st.d_class, (size_t)e->n);
    RESERVE(e, st.d_bits, bits.size());
    RESERVE(e, d_first, 1);
    HIPCHK(e, hipMemcpy(st.d_class.get(), cls, (size_t)e->n, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(st.d_bits.get(), bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice));
    unsigned long long first = ~0ull;
    HIPCHK(e, hipMemcpy(d_first.get(), &first, sizeof(first), hipMemcpyHostToDevice));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (the labels are those of the calls made so far)
    const uint32_t tiles = (uint32_t)std::min<uint64_t>((e->n + 255) / 256, 1024);
    hipLaunchKernelGGL(constraints_check_kernel, dim3(tiles ? tiles : 1, e->n_chains), dim3(256), 0, e->stream, e->d_labels, e->label_stride,
                       (uint32_t)e->n, e->n_chains, st.d_class.get(), st.d_bits.get(), d_first.get());
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(&first, d_first.get(), sizeof(first), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (first != ~0ull) {
        const uint64_t c = first / e->n, v = first % e->n;
        uint8_t lab = 0;
        HIPCHK(e, hipMemcpy(&lab, e->d_labels + (size_t)c * e->label_stride + v, 1, hipMemcpyDeviceToHost));
        return fail(e, BISBM_ERR_STATE, "chain %u holds node %llu in block %u, which its class %u does not allow: the constraints must admit every chain's current labels",
                    e->gid((size_t)c), (unsigned long long)v, (unsigned)lab, (unsigned)cls[v]);
    }
    return build_open(e, st, clamp_mask);
}

}  // namespace

int constraints_rebuild_open(bisbm_engine* e, const std::vector<uint8_t>& clamp_mask) {
    if (!e->constraints.n_classes) return BISBM_OK;
    return build_open(e, e->constraints, clamp_mask);
}

}  // namespace bisbm

extern "C" {

int bisbm_constraints_set(bisbm_handle h, uint32_t n_classes, const uint8_t* class_of_node, const uint8_t* allowed) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "block constraints are defined in Philox mode: this handle runs BISBM_RNG_MT19937_COMPAT, the mode of parity with the reference, which has no constraints");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "block constraints serve byte labels only (at most 256 blocks): merge the blocks down first");
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle have different block counts: block constraints need one shape for all chains");
    if (n_classes > 256) return fail(h, BISBM_ERR_INVALID_ARG, "n_classes = %u: a class id is one byte, at most 256 classes", n_classes);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    const uint32_t ka = entries[0]->ka, K = entries[0]->K;
    const uint64_t n = entries[0]->n, na = entries[0]->na;
    const bool clear = n_classes == 0 || !class_of_node || !allowed;
    bool all_free = true;  // every node may sit in every block of its type: "no constraints"
    std::vector<uint32_t> bits;
    std::vector<ConstraintState> staged;
    try {
        if (!clear) {
            bits.assign((size_t)n_classes * kCnWords, 0u);
            for (uint32_t c = 0; c < n_classes; ++c)
                for (uint32_t s = 0; s < K; ++s)
                    if (allowed[(size_t)c * K + s]) bits[(size_t)c * kCnWords + (s >> 5)] |= 1u << (s & 31u);
            for (uint64_t v = 0; v < n; ++v) {
                const uint32_t c = class_of_node[v];
                if (c >= n_classes)
                    return fail(h, BISBM_ERR_INVALID_ARG, "class %u of node %llu: the table has %u class(es)", c, (unsigned long long)v, n_classes);
                for (uint32_t s = v < na ? 0 : ka; all_free && s < (v < na ? ka : K); ++s) all_free = allowed[(size_t)c * K + s] != 0;
            }
        }
        DeviceGuard keep;
        if (clear || all_free) {
            for (bisbm_engine* e : entries) {
                HIPCHK(h, hipSetDevice(e->device));
                HIPCHK(h, hipStreamSynchronize(e->stream));  // (no kernel of this entry reads the old table any more)
                e->constraints = ConstraintState();
            }
            h->constraints = ConstraintState();
            return BISBM_OK;
        }
        staged.resize(entries.size());
        for (size_t i = 0; i < entries.size(); ++i)
            if (int rc = stage(entries[i], staged[i], n_classes, class_of_node, allowed, bits, h->clamp.mask)) {
                if (entries[i] != h) h->err = entries[i]->err;
                return rc;  // (nothing changed: the constraints in place stay on every device)
            }
        for (size_t i = 0; i < entries.size(); ++i) {
            bisbm_engine* e = entries[i];
            HIPCHK(h, hipSetDevice(e->device));
            HIPCHK(h, hipStreamSynchronize(e->stream));
            e->constraints = std::move(staged[i]);
        }
        if (entries[0] != h) {  // a handle over several devices: the host copies for bisbm_constraints_get
            h->constraints = ConstraintState();
            h->constraints.n_classes = n_classes;
            h->constraints.cls = entries[0]->constraints.cls;
            h->constraints.allowed = entries[0]->constraints.allowed;
            h->constraints.bits = bits;
        }
    } catch (...) {
        return fail(h, BISBM_ERR_STATE, "bisbm_constraints_set: out of host memory");
    }
    return BISBM_OK;
}

int bisbm_constraints_get(bisbm_handle h, uint32_t* n_classes_out, uint8_t* class_of_node_out, uint8_t* allowed_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ConstraintState& st = h->constraints;
    if (n_classes_out) *n_classes_out = st.n_classes;
    if (class_of_node_out) {
        if (st.n_classes)
            std::memcpy(class_of_node_out, st.cls.data(), (size_t)h->n);
        else
            std::memset(class_of_node_out, 0, (size_t)h->n);
    }
    if (allowed_out && st.n_classes)
        for (size_t i = 0; i < st.allowed.size(); ++i) allowed_out[i] = st.allowed[i] ? 1 : 0;
    return BISBM_OK;
}

}  // extern "C"
