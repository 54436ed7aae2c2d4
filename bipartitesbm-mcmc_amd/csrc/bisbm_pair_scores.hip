// bisbm_pair_scores.hip -- posterior-predictive pair scores pooled over chains (no reference counterpart: the reference keeps
// one partition and never scores a pair).  For a pair (u, v), u of type a and v of type b, one chain contributes the DC-SBM's
// expected number of edges between the two given its partition,
//     lambda(u, v) = ((double)d(u) * (double)d(v)) * (double)m[b_u][b_v - KA] / ((double)m_r[b_u] * (double)m_r[b_v]),
// 0.0 when either degree is 0; a sample adds the term of every counted chain to the pair's running f64 sum (include/bisbm.h).
// The term does not depend on how a chain numbers its blocks, so the chains pool as they are: no alignment, any mix of shapes.
//
// Kernel: a workgroup owns a tile of kPairTile pairs (8 per lane, accumulators in registers) and a slab of chains; per chain
// it stages the chain's quadrant of m and its m_r in LDS (two buffers: one barrier per chain; read straight from HBM while
// wide), gathers b_u and b_v, looks up, divides, adds.  Consecutive workgroup ids differ in the slab first, and workgroups are
// dealt round-robin over the 8 XCDs, so the workgroups that share an XCD's L2 walk the same slab of chains from its first
// chain on: one chain's label array (N bytes) is fetched into that L2 once and the other tiles' gathers find it there.  The
// pairs are held sorted by (u, v), so the b_u gather of a tile walks a short stretch of the array.  Slab partials go to
// part[slab][pair] with plain stores and a second kernel adds them to the running sums in slab order: no floating-point
// atomics, the order of the additions is fixed by (pairs, chain count, shape).
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kPairLanes = 256, kPairPerLane = kPairTile / kPairLanes;

__global__ __launch_bounds__(256) void pair_degrees_kernel(const uint32_t* rowptr, const uint32_t* u, const uint32_t* v, uint32_t n_pairs,
                                                           double* dd) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t a = u[i], b = v[i];
    dd[i] = (double)(rowptr[a + 1] - rowptr[a]) * (double)(rowptr[b + 1] - rowptr[b]);
}

template <class LabelT, bool IN_LDS>
__global__ __launch_bounds__(256) void pair_scores_kernel(PairScoreParams p) {
    extern __shared__ __align__(16) int32_t tabs[];  // IN_LDS: 2 x {m quadrant [ka][kb], m_r [K]}
    const uint32_t slab = blockIdx.x % p.slabs, tile = blockIdx.x / p.slabs;
    const uint32_t per = (p.n_chains + p.slabs - 1) / p.slabs;
    const uint32_t c0 = min(slab * per, p.n_chains), c1 = min(c0 + per, p.n_chains);
    const uint32_t K = p.ka + p.kb, quad = p.ka * p.kb, tab = quad + K;
    const LabelT* labels = (const LabelT*)p.labels;

    // lane t holds pairs tile * kPairTile + j * 256 + t; past the end: a pair of degree product 0 that is never stored
    uint32_t pu[kPairPerLane], pv[kPairPerLane];
    double dd[kPairPerLane], acc[kPairPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kPairPerLane; ++j) {
        const uint32_t i = tile * kPairTile + j * kPairLanes + threadIdx.x;
        const bool in = i < p.n_pairs;
        pu[j] = in ? p.u[i] : 0u;
        pv[j] = in ? p.v[i] : p.na;
        dd[j] = in ? p.dd[i] : 0.;
        acc[j] = 0.;
    }

    uint32_t buf = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        if (p.rung && p.rung[c] != 0u) continue;  // (the same for every lane)
        const int32_t* m_g = p.m + (size_t)c * quad;
        const int32_t* mr_g = p.m_r + (size_t)c * K;
        const int32_t *m_t = m_g, *mr_t = mr_g;
        if constexpr (IN_LDS) {
            // the buffer the chain before last used: every wave has passed the barrier of the last chain since it read it
            int32_t* t = tabs + buf * tab;
            for (uint32_t i = threadIdx.x; i < quad; i += kPairLanes) t[i] = m_g[i];
            for (uint32_t i = threadIdx.x; i < K; i += kPairLanes) t[quad + i] = mr_g[i];
            __syncthreads();
            m_t = t, mr_t = t + quad;
            buf ^= 1u;
        }
        const LabelT* lab = labels + (size_t)c * p.label_stride;
        uint32_t bu[kPairPerLane], bv[kPairPerLane];
#pragma unroll
        for (uint32_t j = 0; j < kPairPerLane; ++j) bu[j] = lab[pu[j]], bv[j] = lab[pv[j]];
#pragma unroll
        for (uint32_t j = 0; j < kPairPerLane; ++j) {
            const double mm = (double)m_t[bu[j] * p.kb + (bv[j] - p.ka)];
            const double den = (double)mr_t[bu[j]] * (double)mr_t[bv[j]];
            if (dd[j] != 0.) acc[j] += (dd[j] * mm) / den;  // (d > 0 on both sides: m_r >= d > 0, no division by zero)
        }
    }
    double* out = p.part + (size_t)slab * p.n_pairs;
#pragma unroll
    for (uint32_t j = 0; j < kPairPerLane; ++j) {
        const uint32_t i = tile * kPairTile + j * kPairLanes + threadIdx.x;
        if (i < p.n_pairs) out[i] = acc[j];
    }
}

__global__ __launch_bounds__(256) void pair_scores_fold_kernel(double* sum, const double* part, uint32_t slabs, uint32_t n_pairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    double s = sum[i];
    for (uint32_t k = 0; k < slabs; ++k) s += part[(size_t)k * n_pairs + i];
    sum[i] = s;
}

}  // namespace

namespace bisbm {

// Slabs of a launch: 8 (one per XCD) where there are that many chains, doubled while the tiles alone leave most of the chip
// idle (few pairs, many chains); never more slabs than chains.
uint32_t pair_score_slabs(uint64_t n_pairs, uint32_t n_chains) {
    if (n_chains < 8) return std::max(n_chains, 1u);
    const uint64_t tiles = (n_pairs + kPairTile - 1) / kPairTile;
    uint32_t slabs = 8;
    while (tiles * slabs < 1024 && slabs * 2 <= std::min(n_chains, 64u)) slabs *= 2;
    return slabs;
}

hipError_t launch_pair_degrees(const uint32_t* rowptr, const uint32_t* u, const uint32_t* v, uint32_t n_pairs, double* dd, hipStream_t stream) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(pair_degrees_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, rowptr, u, v, n_pairs, dd);
    return hipGetLastError();
}

hipError_t launch_pair_scores(const PairScoreParams& p, hipStream_t stream) {
    if (p.n_pairs == 0) return hipSuccess;
    const uint32_t tiles = (p.n_pairs + kPairTile - 1) / kPairTile;
    const dim3 grid(tiles * p.slabs), block(kPairLanes);
    if (p.wide) {
        hipLaunchKernelGGL((pair_scores_kernel<uint16_t, false>), grid, block, 0, stream, p);
        return hipGetLastError();
    }
    // byte labels: at most 256 blocks, so two copies of a chain's tables are at most 2 x (64 KiB + 1 KiB) of the CU's 160 KiB
    const size_t lds = sizeof(int32_t) * 2 * ((size_t)p.ka * p.kb + p.ka + p.kb);
    hipError_t e = hipFuncSetAttribute((const void*)pair_scores_kernel<uint8_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pair_scores_kernel<uint8_t, true>), grid, block, lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_pair_scores_fold(double* sum, const double* part, uint32_t slabs, uint32_t n_pairs, hipStream_t stream) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(pair_scores_fold_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, sum, part, slabs, n_pairs);
    return hipGetLastError();
}

}  // namespace bisbm

namespace {

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream
int add_sample(bisbm_engine* h, bisbm_engine* e) {
    PairScoreState& s = h->pairs;
    if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_pair_scores_accumulate");
    const uint32_t slabs = pair_score_slabs(s.n, e->n_chains);
    RESERVE(h, s.d_part, (size_t)slabs * s.n);
    PairScoreParams p{};
    p.n_pairs = (uint32_t)s.n;
    p.na = (uint32_t)h->na;
    p.ka = e->ka;
    p.kb = e->kb;
    p.n_chains = e->n_chains;
    p.slabs = slabs;
    p.u = s.d_u.get();
    p.v = s.d_v.get();
    p.dd = s.d_dd.get();
    p.labels = e->d_labels;
    p.label_stride = e->label_stride;
    p.wide = e->wide ? 1u : 0u;
    p.m = e->d_m;
    p.m_r = e->d_m_r;
    p.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    p.part = s.d_part.get();
    HIPCHK(h, launch_pair_scores(p, h->stream));
    HIPCHK(h, launch_pair_scores_fold(s.d_sum.get(), s.d_part.get(), slabs, p.n_pairs, h->stream));
    s.terms += e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_pair_scores_set(bisbm_handle h, uint64_t n_pairs, const uint32_t* u, const uint32_t* v) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (n_pairs && (!u || !v)) return fail(h, BISBM_ERR_INVALID_ARG, "u or v is NULL");
    if (n_pairs >= 0xFFFFFFFFull) return fail(h, BISBM_ERR_UNSUPPORTED, "more than 2^32-2 pairs");
    for (uint64_t i = 0; i < n_pairs; ++i)  // (before anything changes: a refused call leaves the earlier pairs in place)
        if (u[i] >= h->na || v[i] < h->na || v[i] >= h->n)
            return fail(h, BISBM_ERR_INVALID_ARG, "pair %llu = (%u, %u): u must be a type-a node [0, %llu), v a type-b node [%llu, %llu)",
                        (unsigned long long)i, u[i], v[i], (unsigned long long)h->na, (unsigned long long)h->na, (unsigned long long)h->n);
    if (!h->devs.empty()) {
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_pair_scores_set(d, n_pairs, u, v); });
        h->pairs.n = rc ? 0 : n_pairs;
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pairs = PairScoreState();  // (the old pairs, their sums and buffers go)
    if (n_pairs == 0) return BISBM_OK;
    PairScoreState& s = h->pairs;
    // sorted by (u, v), equal pairs in the caller's order
    std::vector<std::pair<uint64_t, uint32_t>> keyed((size_t)n_pairs);
    for (uint64_t i = 0; i < n_pairs; ++i) keyed[i] = {(uint64_t)u[i] << 32 | v[i], (uint32_t)i};
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> su((size_t)n_pairs), sv((size_t)n_pairs);
    s.order.resize((size_t)n_pairs);
    for (size_t i = 0; i < keyed.size(); ++i) su[i] = (uint32_t)(keyed[i].first >> 32), sv[i] = (uint32_t)keyed[i].first, s.order[i] = keyed[i].second;
    hipError_t e = s.d_u.reserve((size_t)n_pairs);
    if (e == hipSuccess) e = s.d_v.reserve((size_t)n_pairs);
    if (e == hipSuccess) e = s.d_dd.reserve((size_t)n_pairs);
    if (e == hipSuccess) e = s.d_sum.reserve((size_t)n_pairs);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_u.get(), su.data(), sizeof(uint32_t) * n_pairs, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_v.get(), sv.data(), sizeof(uint32_t) * n_pairs, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_sum.get(), 0, sizeof(double) * n_pairs, h->stream);
    if (e == hipSuccess) e = launch_pair_degrees(h->d_rowptr, s.d_u.get(), s.d_v.get(), (uint32_t)n_pairs, s.d_dd.get(), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->pairs = PairScoreState();
        return fail(h, BISBM_ERR_HIP, "bisbm_pair_scores_set: %s", hipGetErrorString(e));
    }
    s.n = n_pairs;
    return BISBM_OK;
}

int bisbm_pair_scores_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->pairs.n) return fail(h, BISBM_ERR_STATE, "no pairs to score: call bisbm_pair_scores_set first");
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_pair_scores_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_pair_scores_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_pair_scores_reset(d); });
    h->pairs.terms = 0;
    if (!h->pairs.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->pairs.d_sum.get(), 0, sizeof(double) * h->pairs.n, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_pair_scores_get(bisbm_handle h, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->pairs.n) return fail(h, BISBM_ERR_STATE, "no pairs to score: call bisbm_pair_scores_set first");
    const size_t P = (size_t)h->pairs.n;
    if (!h->devs.empty()) {  // the per-device sums are added on the host in device order
        std::vector<double> part(sum_out ? P : 0);
        uint64_t terms = 0;
        if (sum_out) std::fill(sum_out, sum_out + P, 0.);
        for (bisbm_engine* d : h->devs) {
            uint64_t t = 0;
            if (int rc = bisbm_pair_scores_get(d, sum_out ? part.data() : nullptr, &t)) {
                h->err = d->err;
                return rc;
            }
            terms += t;
            if (sum_out)
                for (size_t i = 0; i < P; ++i) sum_out[i] += part[i];
        }
        if (terms_out) *terms_out = terms;
        return BISBM_OK;
    }
    if (terms_out) *terms_out = h->pairs.terms;
    if (!sum_out) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<double> sorted(P);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(sorted.data(), h->pairs.d_sum.get(), sizeof(double) * P, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < P; ++i) sum_out[h->pairs.order[i]] = sorted[i];
    return BISBM_OK;
}

}  // extern "C"
