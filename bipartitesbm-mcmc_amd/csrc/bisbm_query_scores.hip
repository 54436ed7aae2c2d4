// bisbm_query_scores.hip -- query scores: every candidate of a node scored over the chains; the best k of them are selected on
// the device by bisbm_topk.hip (no reference counterpart; include/bisbm.h, "Query scores").  A query is a node q of either type,
// its candidates are all nodes of the other type in id order, and one chain's term for (query, candidate) is the pair-score term
// of the pair (type-a node u, type-b node v) the two form,
//     ((double)d(u) * (double)d(v)) * (double)m[b_u][b_v - KA] / ((double)m_r[b_u] * (double)m_r[b_v]),
// 0.0 when either degree is 0 (bisbm_pair_scores.hip).  The two products commute exactly, so a type-b query only swaps which
// index of m the query's label takes.
//
// Accumulate kernel: a workgroup owns kQueryCandTile candidates x kQueryTile queries of one type (bisbm_cand_lanes.hpp), keeps the
// 4 x 8 running sums of a lane in registers and walks ALL counted chains in ascending order, one f64 add per chain onto the
// running sum: the bits do not depend on the launch geometry.  Per chain it stages only the queries' rows (columns, for type-b
// queries) of the chain's quadrant of m, the other type's m_r and the queries' own m_r in LDS (two buffers: one barrier per chain).
//
// Top-k: the selection of bisbm_topk.hip on the bit patterns of the sums; with the neighbours left out, a query's CSR row is the
// list that masks.
#include "bisbm_cand_lanes.hpp"
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256, kRowStride = 256;  // (a type has at most 255 blocks while the labels are bytes)
constexpr uint32_t kTabInts = kQueryTile * kRowStride + kRowStride + kQueryTile;  // m rows | m_r of the candidates' type | m_r of the queries

template <bool TYPE_B>
__global__ __launch_bounds__(256) void query_scores_kernel(QueryScoreParams p) {
    __shared__ int32_t tabs[2][kTabInts];
    __shared__ uint32_t q_node[kQueryTile];
    __shared__ double q_deg[kQueryTile];
    const uint32_t first = TYPE_B ? 0u : p.na, n_other = TYPE_B ? p.na : p.n - p.na;
    const uint32_t k_oth = TYPE_B ? p.ka : p.kb, lab_oth = TYPE_B ? 0u : p.ka, lab_own = TYPE_B ? p.ka : 0u;
    const uint32_t cand_tile = blockIdx.x % p.cand_tiles, q0 = (p.q_tile0 + blockIdx.x / p.cand_tiles) * kQueryTile;
    const uint32_t nq = min(kQueryTile, p.n_list - q0);
    const uint32_t K = p.ka + p.kb, quad = p.ka * p.kb;

    const CandLanes cl = cand_lanes(first, n_other, cand_tile);
    double dv[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) dv[j] = cl.valid[j] ? (double)(p.rowptr[cl.node(j) + 1] - p.rowptr[cl.node(j)]) : 0.;
    if (threadIdx.x < nq) {
        const uint32_t q = p.queries[p.list[q0 + threadIdx.x]];
        q_node[threadIdx.x] = q;
        q_deg[threadIdx.x] = (double)(p.rowptr[q + 1] - p.rowptr[q]);
    }
    double acc[kQueryTile][4];
#pragma unroll
    for (uint32_t i = 0; i < kQueryTile; ++i) {
        const double* row = i < nq ? p.sum + p.off[p.list[q0 + i]] : nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = (i < nq && cl.valid[j]) ? row[cl.node(j) - first] : 0.;
    }
    __syncthreads();

    uint32_t buf = 0;
    for (uint32_t c = 0; c < p.n_chains; ++c) {
        if (p.rung && p.rung[c] != 0u) continue;  // (the same for every lane)
        const int32_t* m_g = p.m + (size_t)c * quad;
        const int32_t* mr_g = p.m_r + (size_t)c * K;
        const uint8_t* lab = p.labels + (size_t)c * p.label_stride;
        // the buffer the chain before last used: every wave has passed the barrier of the last chain since it read it
        int32_t* t = tabs[buf];
        for (uint32_t i = threadIdx.x; i < nq * k_oth; i += kLanes) {
            const uint32_t qi = i / k_oth, x = i - qi * k_oth, b = (uint32_t)lab[q_node[qi]] - lab_own;
            t[qi * kRowStride + x] = TYPE_B ? m_g[x * p.kb + b] : m_g[b * p.kb + x];
        }
        for (uint32_t i = threadIdx.x; i < k_oth; i += kLanes) t[kQueryTile * kRowStride + i] = mr_g[lab_oth + i];
        if (threadIdx.x < nq) t[kQueryTile * kRowStride + kRowStride + threadIdx.x] = mr_g[lab[q_node[threadIdx.x]]];
        __syncthreads();
        buf ^= 1u;
        const uint32_t word = cl.any ? *(const uint32_t*)(lab + (size_t)cl.w * 4) : 0u;
        uint32_t bv[4];
        double mrv[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            bv[j] = cl.valid[j] ? ((word >> (8 * j)) & 255u) - lab_oth : 0u;
            mrv[j] = (double)t[kQueryTile * kRowStride + bv[j]];
        }
#pragma unroll
        for (uint32_t i = 0; i < kQueryTile; ++i) {
            if (i >= nq) break;  // (the same for every lane)
            const double mrq = (double)t[kQueryTile * kRowStride + kRowStride + i], dq = q_deg[i];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                // u is the type-a node of the two: the query, or with type-b queries the candidate
                const double dd = TYPE_B ? dv[j] * dq : dq * dv[j];
                const double mm = (double)t[i * kRowStride + bv[j]];
                const double den = TYPE_B ? mrv[j] * mrq : mrq * mrv[j];
                if (dd != 0.) acc[i][j] += (dd * mm) / den;  // (d > 0 on both sides: m_r >= d > 0, no division by zero)
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kQueryTile; ++i) {
        if (i >= nq) break;
        double* row = p.sum + p.off[p.list[q0 + i]];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (cl.valid[j]) row[cl.node(j) - first] = acc[i][j];
    }
}

}  // namespace

namespace bisbm {

hipError_t launch_query_scores(const QueryScoreParams& p_in, hipStream_t stream) {
    QueryScoreParams p = p_in;
    if (p.n_list == 0) return hipSuccess;
    const uint64_t first = p.type ? 0u : p.na, n_other = p.type ? p.na : p.n - p.na;
    if (n_other == 0) return hipSuccess;
    return for_cand_grids(first, n_other, p.n_list, kQueryTile, [&](uint32_t cand_tiles, uint32_t q_tile0, dim3 grid) {
        p.cand_tiles = cand_tiles, p.q_tile0 = q_tile0;
        if (p.type)
            hipLaunchKernelGGL(query_scores_kernel<true>, grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL(query_scores_kernel<false>, grid, dim3(kLanes), 0, stream, p);
    });
}

}  // namespace bisbm

namespace {

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream
int add_sample(bisbm_engine* h, bisbm_engine* e) {
    QueryScoreState& s = h->queries;
    QueryScoreParams p{};
    p.n = (uint32_t)h->n;
    p.na = (uint32_t)h->na;
    p.ka = e->ka;
    p.kb = e->kb;
    p.n_chains = e->n_chains;
    p.queries = s.d_q.get();
    p.off = s.d_off.get();
    p.rowptr = h->d_rowptr;
    p.labels = e->d_labels;
    p.label_stride = e->label_stride;
    p.m = e->d_m;
    p.m_r = e->d_m_r;
    p.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    p.sum = s.d_sum.get();
    for (uint32_t type = 0; type < 2; ++type) {
        p.type = type;
        p.n_list = type ? s.n - s.n_a : s.n_a;
        p.list = s.d_list.get() + (type ? s.n_a : 0u);
        HIPCHK(h, launch_query_scores(p, h->stream));
    }
    s.terms += e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    return BISBM_OK;
}

const double* sums_of(bisbm_engine* d) { return d->queries.d_sum.get(); }

}  // namespace

extern "C" {

int bisbm_query_scores_set(bisbm_handle h, uint32_t n_queries, const uint32_t* queries) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (n_queries && !queries) return fail(h, BISBM_ERR_INVALID_ARG, "queries is NULL");
    for (uint32_t i = 0; i < n_queries; ++i)  // (before anything changes: a refused call leaves the earlier queries in place)
        if (queries[i] >= h->n)
            return fail(h, BISBM_ERR_INVALID_ARG, "query %u = %u: not a node [0, %llu)", i, queries[i], (unsigned long long)h->n);
    std::vector<uint32_t> q(queries, queries + n_queries), list;
    std::vector<uint64_t> off((size_t)n_queries + 1, 0);
    std::vector<TopkCand> cand(n_queries);  // the candidates: the other type's nodes, every one of them eligible
    const uint32_t n_a = partition_by_type(q, h->na, list);
    for (uint32_t i = 0; i < n_queries; ++i) {
        off[i + 1] = off[i] + (q[i] < h->na ? h->nb : h->na);
        cand[i] = TopkCand{q[i] < h->na ? (uint32_t)h->na : 0u, 0xffffffffu};
    }
    if (!h->devs.empty()) {
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_query_scores_set(d, n_queries, queries); });
        h->queries = QueryScoreState();
        if (rc == BISBM_OK && n_queries) h->queries.n = n_queries, h->queries.n_a = n_a, h->queries.q = q, h->queries.off = off;
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->queries = QueryScoreState();  // (the old queries, their sums and buffers go)
    if (n_queries == 0) return BISBM_OK;
    QueryScoreState& s = h->queries;
    const size_t cells = (size_t)off[n_queries];
    hipError_t e = s.d_sum.reserve(cells);
    if (e != hipSuccess) {
        h->queries = QueryScoreState();
        return fail(h, BISBM_ERR_HIP, "bisbm_query_scores_set: %zu bytes of device memory for the sums of %u queries could not be allocated: %s",
                    cells * sizeof(double), n_queries, hipGetErrorString(e));
    }
    e = s.d_q.reserve(n_queries);
    if (e == hipSuccess) e = s.d_off.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = s.d_list.reserve(n_queries);
    if (e == hipSuccess) e = s.d_cand.reserve(n_queries);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_q.get(), q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off.get(), off.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_list.get(), list.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_cand.get(), cand.data(), sizeof(TopkCand) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_sum.get(), 0, sizeof(double) * cells, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->queries = QueryScoreState();
        return fail(h, BISBM_ERR_HIP, "bisbm_query_scores_set: %s", hipGetErrorString(e));
    }
    s.n = n_queries, s.n_a = n_a;
    s.q.swap(q), s.off.swap(off);
    return BISBM_OK;
}

int bisbm_query_scores_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->queries.n) return fail(h, BISBM_ERR_STATE, "no queries to score: call bisbm_query_scores_set first");
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED,
                    "query scores serve byte labels only (at most 256 blocks); bisbm_pair_scores_* serves two-byte labels: list the pairs there");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_query_scores_accumulate");
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_query_scores_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_query_scores_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_query_scores_reset(d); });
    h->queries.terms = 0;
    if (!h->queries.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->queries.d_sum.get(), 0, sizeof(double) * h->queries.off[h->queries.n], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_query_scores_get_row(bisbm_handle h, uint32_t query_index, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const QueryScoreState& s = h->queries;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to score: call bisbm_query_scores_set first");
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u queries are set", query_index, s.n);
    if (terms_out) *terms_out = total_terms(h, &bisbm_engine::queries);
    if (!sum_out) return BISBM_OK;
    return read_row(h, per_device(h, sums_of), s.off[query_index], (size_t)(s.off[query_index + 1] - s.off[query_index]), sum_out);
}

int bisbm_query_scores_topk(bisbm_handle h, uint32_t k, int exclude_neighbours, uint32_t* node_out, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const QueryScoreState& s = h->queries;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to score: call bisbm_query_scores_set first");
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_query_scores_topk selects at most %u candidates per query", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h, &bisbm_engine::queries);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_query_scores_accumulate before bisbm_query_scores_topk");
    if (terms_out) *terms_out = terms;
    bisbm_engine* e = device_entries(h)[0];  // the device that selects
    QueryScoreState& w = e->queries;
    const TopkMaskLists neighbours{e->d_rowptr, nullptr, w.d_q.get(), e->d_col};  // a query's CSR row
    return topk_select(h, __func__, per_device(h, sums_of), s.off, w.topk, w.d_off.get(), w.d_cand.get(), exclude_neighbours ? &neighbours : nullptr, k,
                       node_out, sum_out);
}

}  // extern "C"
