// bisbm_query_scores.hip -- query scores: every candidate of a node scored over the chains, and the best k of them selected on
// the device (no reference counterpart; include/bisbm.h, "Query scores").  A query is a node q of either type, its candidates
// are all nodes of the other type in id order, and one chain's term for (query, candidate) is the pair-score term of the pair
// (type-a node u, type-b node v) the two form,
//     ((double)d(u) * (double)d(v)) * (double)m[b_u][b_v - KA] / ((double)m_r[b_u] * (double)m_r[b_v]),
// 0.0 when either degree is 0 (bisbm_pair_scores.hip).  The two products commute exactly, so a type-b query only swaps which
// index of m the query's label takes.
//
// Accumulate kernel: a workgroup owns kQueryCandTile candidates (a lane reads its four labels as one word of the chain's label
// row: coalesced) x kQueryTile queries of one type, keeps the 4 x 8 running sums of a lane in registers and walks ALL counted
// chains in ascending order, one f64 add per chain onto the running sum: the bits do not depend on the launch geometry.  Per chain
// it stages only the queries' rows (columns, for type-b queries) of the chain's quadrant of m, the other type's m_r and the
// queries' own m_r in LDS (two buffers: one barrier per chain).  No two workgroups share a cell of `sum`.
//
// Top-k: a neighbour mask over the candidates of a chunk of queries (one byte per cell), then one workgroup per query: the sums
// are non-negative, so their bit patterns order as uint64 -- an exact radix select (8 passes of 8 bits) of the k-th largest
// eligible key, an ordered compaction (ballots and wave offsets, no atomics order) of the larger keys and of the first ties in
// id order, and a rank sort of the k entries by (key descending, id ascending).
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

    // lane t holds the four nodes of label word w; the ones outside the candidates are never looked up or stored
    const uint32_t w = (first >> 2) + cand_tile * kLanes + threadIdx.x;
    const bool any = (uint64_t)w * 4 < (uint64_t)first + n_other;
    bool valid[4];
    double dv[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t v = (uint64_t)w * 4 + j;
        valid[j] = v >= first && v < (uint64_t)first + n_other;
        dv[j] = valid[j] ? (double)(p.rowptr[v + 1] - p.rowptr[v]) : 0.;
    }
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
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = (i < nq && valid[j]) ? row[(uint64_t)w * 4 + j - first] : 0.;
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
        const uint32_t word = any ? *(const uint32_t*)(lab + (size_t)w * 4) : 0u;
        uint32_t bv[4];
        double mrv[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            bv[j] = valid[j] ? ((word >> (8 * j)) & 255u) - lab_oth : 0u;
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
            if (valid[j]) row[(uint64_t)w * 4 + j - first] = acc[i][j];
    }
}

// one workgroup per query of the chunk: every entry of its CSR row marks its cell (a multi-edge marks it again)
__global__ __launch_bounds__(256) void query_mask_kernel(const uint32_t* rowptr, const uint32_t* col, QuerySelectParams p, uint8_t* mask) {
    const uint32_t qi = p.q0 + blockIdx.x, q = p.queries[qi];
    const uint32_t first = q < p.na ? p.na : 0u, n_other = q < p.na ? p.n - p.na : p.na;
    uint8_t* row = mask + (p.off[qi] - p.off[p.q0]);
    for (uint32_t e = rowptr[q] + threadIdx.x; e < rowptr[q + 1]; e += blockDim.x) {
        const uint32_t x = col[e] - first;
        if (x < n_other) row[x] = 1;
    }
}

__global__ __launch_bounds__(256) void query_select_kernel(QuerySelectParams p) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[2][2][kLanes / 64];
    __shared__ unsigned long long s_key[kQueryMaxK];
    __shared__ uint32_t s_id[kQueryMaxK];
    __shared__ unsigned long long s_prefix;
    __shared__ uint32_t s_remaining, s_eligible;
    const uint32_t qi = p.q0 + blockIdx.x, q = p.queries[qi];
    const uint32_t first = q < p.na ? p.na : 0u, n_other = q < p.na ? p.n - p.na : p.na;
    const uint64_t cell0 = p.off[qi] - p.off[p.q0];
    const unsigned long long* key = (const unsigned long long*)(p.rows + cell0);
    const uint8_t* mask = p.mask ? p.mask + cell0 : nullptr;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* node_out = p.node_out + (size_t)blockIdx.x * p.k;
    double* sum_out = p.sum_out + (size_t)blockIdx.x * p.k;

    if (tid == 0) s_eligible = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_other; i += kLanes) mine += !(mask && mask[i]);
    if (mine) atomicAdd(&s_eligible, mine);
    __syncthreads();
    const uint32_t kk = min(p.k, s_eligible);
    for (uint32_t e = kk + tid; e < p.k; e += kLanes) node_out[e] = 0xffffffffu, sum_out[e] = 0.;
    if (kk == 0) return;

    // the kk-th largest eligible key, byte by byte from the top: `prefix` holds the bytes found, `remaining` the rank within them
    if (tid == 0) s_prefix = 0, s_remaining = kk;
    for (int b = 7; b >= 0; --b) {
        hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (uint32_t i = tid; i < n_other; i += kLanes) {
            if (mask && mask[i]) continue;
            const unsigned long long x = key[i];
            if (b == 7 || (x >> (8 * (b + 1))) == (prefix >> (8 * (b + 1)))) atomicAdd(&hist[(x >> (8 * b)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rem = s_remaining, bin = 255;
            while (bin > 0 && hist[bin] < rem) rem -= hist[bin], --bin;  // (the bins hold at least `rem` keys in all)
            s_remaining = rem;
            s_prefix = prefix | ((unsigned long long)bin << (8 * b));
        }
        __syncthreads();
    }
    const unsigned long long kth = s_prefix;
    const uint32_t n_ties = s_remaining, n_greater = kk - n_ties;  // ties to take (>= 1), keys above the k-th

    // ordered compaction: the larger keys into [0, n_greater), the first n_ties ties in id order behind them
    uint32_t g_base = 0, t_base = 0, it = 0;
    for (uint32_t s = 0; s < n_other && (g_base < n_greater || t_base < n_ties); s += kLanes, it ^= 1u) {
        const uint32_t i = s + tid;
        const bool in = i < n_other && !(mask && mask[i]);
        const unsigned long long x = in ? key[i] : 0ull;
        const bool isg = in && x > kth, ist = in && x == kth;
        const unsigned long long bg = __ballot(isg), bt = __ballot(ist), below = (1ull << lane) - 1ull;
        if (lane == 0) wsum[it][0][wave] = (uint32_t)__popcll(bg), wsum[it][1][wave] = (uint32_t)__popcll(bt);
        __syncthreads();  // (the other buffer is written next: one barrier per chunk)
        uint32_t g_off = 0, t_off = 0, g_all = 0, t_all = 0;
        for (uint32_t k = 0; k < kLanes / 64; ++k) {
            if (k < wave) g_off += wsum[it][0][k], t_off += wsum[it][1][k];
            g_all += wsum[it][0][k], t_all += wsum[it][1][k];
        }
        if (isg) {
            const uint32_t pos = g_base + g_off + (uint32_t)__popcll(bg & below);
            if (pos < n_greater) s_key[pos] = x, s_id[pos] = i;
        }
        if (ist) {
            const uint32_t pos = t_base + t_off + (uint32_t)__popcll(bt & below);
            if (pos < n_ties) s_key[n_greater + pos] = x, s_id[n_greater + pos] = i;
        }
        g_base += g_all, t_base += t_all;
    }
    __syncthreads();

    // rank of every entry among the kk: (key descending, id ascending); the ids differ, so the ranks are a permutation
    for (uint32_t e = tid; e < kk; e += kLanes) {
        const unsigned long long x = s_key[e];
        const uint32_t id = s_id[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < kk; ++j) rank += (s_key[j] > x) || (s_key[j] == x && s_id[j] < id);
        node_out[rank] = first + id;
        sum_out[rank] = __longlong_as_double((long long)x);
    }
}

__global__ __launch_bounds__(256) void query_rows_add_kernel(double* a, const double* b, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) a[i] += b[i];
}

}  // namespace

namespace bisbm {

hipError_t launch_query_scores(const QueryScoreParams& p_in, hipStream_t stream) {
    QueryScoreParams p = p_in;
    if (p.n_list == 0) return hipSuccess;
    const uint64_t first = p.type ? 0u : p.na, n_other = p.type ? p.na : p.n - p.na;
    if (n_other == 0) return hipSuccess;
    const uint64_t words = ((first + n_other - 1) >> 2) - (first >> 2) + 1;
    p.cand_tiles = (uint32_t)((words + kLanes - 1) / kLanes);
    // workgroup = candidate tile + cand_tiles * query tile: neighbours in the grid walk neighbouring stretches of the same label
    // rows for the same queries; as many query tiles per launch as a one-dimensional grid holds
    const uint32_t q_tiles = (p.n_list + kQueryTile - 1) / kQueryTile, per_launch = std::max(1u, (1u << 30) / p.cand_tiles);
    for (p.q_tile0 = 0; p.q_tile0 < q_tiles; p.q_tile0 += per_launch) {
        const dim3 grid(p.cand_tiles * std::min(per_launch, q_tiles - p.q_tile0));
        if (p.type)
            hipLaunchKernelGGL(query_scores_kernel<true>, grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL(query_scores_kernel<false>, grid, dim3(kLanes), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_query_mask(const uint32_t* rowptr, const uint32_t* col, const QuerySelectParams& p, uint8_t* mask, hipStream_t stream) {
    if (p.n_q == 0) return hipSuccess;
    hipLaunchKernelGGL(query_mask_kernel, dim3(p.n_q), dim3(256), 0, stream, rowptr, col, p, mask);
    return hipGetLastError();
}

hipError_t launch_query_select(const QuerySelectParams& p, hipStream_t stream) {
    if (p.n_q == 0) return hipSuccess;
    hipLaunchKernelGGL(query_select_kernel, dim3(p.n_q), dim3(kLanes), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_query_rows_add(double* a, const double* b, uint64_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(query_rows_add_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, a, b, count);
    return hipGetLastError();
}

}  // namespace bisbm

namespace {

constexpr uint64_t kTopkChunkCells = 1ull << 24;  // cells of one chunk of queries in bisbm_query_scores_topk (at least one query)

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

uint64_t total_terms(bisbm_engine* h) {
    uint64_t t = 0;
    for (bisbm_engine* d : device_entries(h)) t += d->queries.terms;
    return t;
}

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
    uint32_t n_a = 0;
    for (uint32_t i = 0; i < n_queries; ++i) {
        off[i + 1] = off[i] + (q[i] < h->na ? h->nb : h->na);
        if (q[i] < h->na) list.push_back(i), ++n_a;
    }
    for (uint32_t i = 0; i < n_queries; ++i)
        if (q[i] >= h->na) list.push_back(i);
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
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_q.get(), q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off.get(), off.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_list.get(), list.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
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
    if (terms_out) *terms_out = total_terms(h);
    if (!sum_out) return BISBM_OK;
    const size_t len = (size_t)(s.off[query_index + 1] - s.off[query_index]);
    DeviceGuard keep;
    std::vector<double> part(h->devs.empty() ? 0 : len);
    bool first = true;
    for (bisbm_engine* d : device_entries(h)) {  // (several devices: the device rows are added on the host in device order)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        double* dst = h->devs.empty() ? sum_out : part.data();
        HIPCHK(h, hipMemcpy(dst, d->queries.d_sum.get() + s.off[query_index], sizeof(double) * len, hipMemcpyDeviceToHost));
        if (!h->devs.empty())
            for (size_t i = 0; i < len; ++i) sum_out[i] = first ? part[i] : sum_out[i] + part[i];
        first = false;
    }
    return BISBM_OK;
}

int bisbm_query_scores_topk(bisbm_handle h, uint32_t k, int exclude_neighbours, uint32_t* node_out, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const QueryScoreState& s = h->queries;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to score: call bisbm_query_scores_set first");
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_query_scores_topk selects at most %u candidates per query", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_query_scores_accumulate before bisbm_query_scores_topk");
    if (terms_out) *terms_out = terms;
    const std::vector<bisbm_engine*> entries = device_entries(h);
    bisbm_engine* e = entries[0];  // the device that selects
    QueryScoreState& w = e->queries;
    DeviceGuard keep;
    for (bisbm_engine* d : entries) {  // (the sums of every device are complete)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
    }
    HIPCHK(h, hipSetDevice(e->device));
    for (uint32_t q0 = 0; q0 < s.n;) {
        uint32_t q1 = q0 + 1;
        while (q1 < s.n && s.off[q1 + 1] - s.off[q0] <= kTopkChunkCells) ++q1;
        const size_t cells = (size_t)(s.off[q1] - s.off[q0]), n_q = q1 - q0;
        QuerySelectParams p{};
        p.n = (uint32_t)h->n, p.na = (uint32_t)h->na, p.q0 = q0, p.n_q = (uint32_t)n_q, p.k = k;
        p.queries = w.d_q.get();
        p.off = w.d_off.get();
        p.rows = w.d_sum.get() + s.off[q0];
        if (entries.size() > 1) {  // the other devices' rows are added onto a copy of the first device's, in device order
            RESERVE(h, w.d_rows, cells);
            RESERVE(h, w.d_stage, cells);
            HIPCHK(h, hipMemcpyAsync(w.d_rows.get(), p.rows, sizeof(double) * cells, hipMemcpyDeviceToDevice, e->stream));
            for (size_t j = 1; j < entries.size(); ++j) {
                HIPCHK(h, hipMemcpyPeerAsync(w.d_stage.get(), e->device, entries[j]->queries.d_sum.get() + s.off[q0], entries[j]->device,
                                             sizeof(double) * cells, e->stream));
                HIPCHK(h, launch_query_rows_add(w.d_rows.get(), w.d_stage.get(), cells, e->stream));
            }
            p.rows = w.d_rows.get();
        }
        if (exclude_neighbours) {
            RESERVE(h, w.d_mask, cells);
            HIPCHK(h, hipMemsetAsync(w.d_mask.get(), 0, cells, e->stream));
            HIPCHK(h, launch_query_mask(e->d_rowptr, e->d_col, p, w.d_mask.get(), e->stream));
            p.mask = w.d_mask.get();
        }
        RESERVE(h, w.d_node, n_q * k);
        RESERVE(h, w.d_val, n_q * k);
        p.node_out = w.d_node.get();
        p.sum_out = w.d_val.get();
        HIPCHK(h, launch_query_select(p, e->stream));
        HIPCHK(h, hipMemcpyAsync(node_out + (size_t)q0 * k, w.d_node.get(), sizeof(uint32_t) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        if (sum_out) HIPCHK(h, hipMemcpyAsync(sum_out + (size_t)q0 * k, w.d_val.get(), sizeof(double) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(h, hipStreamSynchronize(e->stream));  // (the scratch is reused by the next chunk)
        q0 = q1;
    }
    return BISBM_OK;
}

}  // extern "C"
