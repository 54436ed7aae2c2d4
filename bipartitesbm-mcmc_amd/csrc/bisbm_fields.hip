// bisbm_fields.hip -- block fields: a class byte per node and a table of f64 energies phi[class][block] in nats; with
// Phi(b) = sum_v phi[class(v)][b_v] every sampler targets exp(-beta (S + Phi)) (no reference counterpart; include/bisbm.h,
// "Block fields", states what every sampler does with them).  This unit keeps the state -- the host copies, and on every device
// entry the class bytes and the table -- and computes Phi per chain.  The kernels that read the table are the samplers' own:
// sweep_kernel (bisbm_kernels.hip), heatbath_kernel (bisbm_heatbath.hip), reshuffle_kernel (bisbm_reshuffle.hip); each is handed
// the pointers only while fields are set (FieldState::field_or_null), so a handle without fields runs what it ran before.
#include "bisbm_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace bisbm;

namespace bisbm {

namespace {

// Phi of one chain per workgroup.  The integer histogram count[class][block] over the nodes goes through LDS, `tile` classes at
// a time (integer adds: their order is free); then one lane adds (double)count * phi over (class ascending, block ascending),
// zero counts skipped, which is the order of the definition -- a label is a block of its node's type, so a count outside the own
// type's range is zero.  The tiles are walked in ascending class order, so tiling does not change the sum.
__global__ __launch_bounds__(256) void fields_energy_kernel(const uint8_t* labels, size_t label_stride, uint32_t n, uint32_t K, uint32_t n_chains,
                                                            const uint8_t* cls, const double* field, uint32_t n_classes, uint32_t tile, double* out) {
    extern __shared__ uint32_t s_count[];  // [tile][K]
    const uint32_t chain = blockIdx.x;
    if (chain >= n_chains) return;
    const uint8_t* lab = labels + (size_t)chain * label_stride;
    double phi = 0.;
    for (uint32_t c0 = 0; c0 < n_classes; c0 += tile) {
        const uint32_t tc = n_classes - c0 < tile ? n_classes - c0 : tile;
        for (uint32_t i = threadIdx.x; i < tc * K; i += blockDim.x) s_count[i] = 0u;
        __syncthreads();
        for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
            const uint32_t c = cls[v], b = lab[v];
            if (c >= c0 && c - c0 < tc && b < K) atomicAdd(&s_count[(c - c0) * K + b], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t c = 0; c < tc; ++c)
                for (uint32_t b = 0; b < K; ++b) {
                    const uint32_t cnt = s_count[c * K + b];
                    if (cnt) phi = phi + (double)cnt * field[(size_t)(c0 + c) * K + b];
                }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[chain] = phi;
}

// 32-bit words of LDS the histogram may take: a tile holds floor(words / K) classes, at least one (K <= 256).
// BISBM_FIELDS_TILE_WORDS, read once, sets it (tests take the tiled path with a small table that way).
uint32_t tile_words() {
    static const uint32_t words = [] {
        const char* env = getenv("BISBM_FIELDS_TILE_WORDS");
        long v = env ? atol(env) : 8192;
        return (uint32_t)std::min<long>(std::max<long>(v, 256), 8192);
    }();
    return words;
}

}  // namespace

int fields_energy_device(bisbm_engine* e) {
    FieldState& st = e->fields;
    HIPCHK(e, hipSetDevice(e->device));
    RESERVE(e, st.d_phi, e->n_chains);
    const uint32_t tile = std::max<uint32_t>(1u, std::min<uint32_t>(st.n_classes, tile_words() / e->K));
    hipLaunchKernelGGL(fields_energy_kernel, dim3(e->n_chains), dim3(256), sizeof(uint32_t) * (size_t)tile * e->K, e->stream, e->d_labels, e->label_stride,
                       (uint32_t)e->n, e->K, e->n_chains, st.d_class.get(), st.d_field.get(), st.n_classes, tile, st.d_phi.get());
    HIPCHK(e, hipGetLastError());
    return BISBM_OK;
}

}  // namespace bisbm

extern "C" {

int bisbm_fields_set(bisbm_handle h, uint32_t n_classes, const uint8_t* class_of_node, const double* field) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "block fields are defined in Philox mode: this handle runs BISBM_RNG_MT19937_COMPAT, the mode of parity with the reference, which has no fields");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "block fields serve byte labels only (at most 256 blocks): merge the blocks down first");
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle have different block counts: block fields need one shape for all chains");
    if (n_classes > 256) return fail(h, BISBM_ERR_INVALID_ARG, "n_classes = %u: a class id is one byte, at most 256 classes", n_classes);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    const uint32_t K = entries[0]->K;
    const uint64_t n = entries[0]->n;
    const bool clear = n_classes == 0 || !class_of_node || !field;
    bool all_zero = true;
    try {
        if (!clear) {
            for (uint32_t c = 0; c < n_classes; ++c)
                for (uint32_t s = 0; s < K; ++s) {
                    const double x = field[(size_t)c * K + s];
                    if (std::isnan(x)) return fail(h, BISBM_ERR_INVALID_ARG, "field[%u][%u] is NaN: every entry must be finite", c, s);
                    if (std::isinf(x) && x > 0.)
                        return fail(h, BISBM_ERR_INVALID_ARG, "field[%u][%u] is +inf: every entry must be finite; bisbm_constraints_set is the way to forbid a block", c, s);
                    if (std::isinf(x)) return fail(h, BISBM_ERR_INVALID_ARG, "field[%u][%u] is -inf: every entry must be finite", c, s);
                    all_zero = all_zero && x == 0.;
                }
            for (uint64_t v = 0; v < n; ++v)
                if (class_of_node[v] >= n_classes)
                    return fail(h, BISBM_ERR_INVALID_ARG, "class %u of node %llu: the table has %u class(es)", (unsigned)class_of_node[v], (unsigned long long)v, n_classes);
        }
        DeviceGuard keep;
        if (clear || all_zero) {
            for (bisbm_engine* e : entries) {
                HIPCHK(h, hipSetDevice(e->device));
                HIPCHK(h, hipStreamSynchronize(e->stream));  // (no kernel of this entry reads the old table any more)
                e->fields = FieldState();
            }
            h->fields = FieldState();
            return BISBM_OK;
        }
        // staged on every device entry first, put in place only when every entry took it: a refusal keeps the fields in place
        std::vector<FieldState> staged(entries.size());
        for (size_t i = 0; i < entries.size(); ++i) {
            bisbm_engine* e = entries[i];
            FieldState& st = staged[i];
            HIPCHK(h, hipSetDevice(e->device));
            st.n_classes = n_classes;
            st.cls.assign(class_of_node, class_of_node + n);
            st.field.assign(field, field + (size_t)n_classes * K);
            RESERVE(h, st.d_class, (size_t)n);
            RESERVE(h, st.d_field, (size_t)n_classes * K);
            HIPCHK(h, hipMemcpy(st.d_class.get(), class_of_node, (size_t)n, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(st.d_field.get(), field, sizeof(double) * (size_t)n_classes * K, hipMemcpyHostToDevice));
        }
        for (size_t i = 0; i < entries.size(); ++i) {
            bisbm_engine* e = entries[i];
            HIPCHK(h, hipSetDevice(e->device));
            HIPCHK(h, hipStreamSynchronize(e->stream));
            e->fields = std::move(staged[i]);
        }
        if (entries[0] != h) {  // a handle over several devices: the host copies for bisbm_fields_get
            h->fields = FieldState();
            h->fields.n_classes = n_classes;
            h->fields.cls = entries[0]->fields.cls;
            h->fields.field = entries[0]->fields.field;
        }
    } catch (...) {
        return fail(h, BISBM_ERR_STATE, "bisbm_fields_set: out of host memory");
    }
    return BISBM_OK;
}

int bisbm_fields_get(bisbm_handle h, uint32_t* n_classes_out, uint8_t* class_of_node_out, double* field_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const FieldState& st = h->fields;
    if (n_classes_out) *n_classes_out = st.n_classes;
    if (class_of_node_out) {
        if (st.n_classes)
            std::memcpy(class_of_node_out, st.cls.data(), (size_t)h->n);
        else
            std::memset(class_of_node_out, 0, (size_t)h->n);
    }
    if (field_out && st.n_classes) std::memcpy(field_out, st.field.data(), sizeof(double) * st.field.size());
    return BISBM_OK;
}

int bisbm_fields_energy(bisbm_handle h, double* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    if (!h->devs.empty()) return on_devices(h, [&](bisbm_engine* d, size_t i) { return bisbm_fields_energy(d, out + h->dev_first[i]); });
    if (!h->fields.n_classes) {  // no fields: Phi = 0
        for (uint32_t c = 0; c < h->n_chains; ++c) out[c] = 0.;
        return BISBM_OK;
    }
    if (!h->state_ready) return fail(h, BISBM_ERR_STATE, "block state not built yet");
    if (int rc = fields_energy_device(h)) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->fields.d_phi.get(), sizeof(double) * h->n_chains, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

}  // extern "C"
