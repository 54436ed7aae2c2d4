// bisbm_edge_queries.hip -- edge queries: every candidate of a node weighed by the exact change of the description length when the
// edge to it is added; the best k are selected on the device by bisbm_topk.hip (no reference counterpart; include/bisbm.h, "Edge
// queries").  A query is a node q of either type, its candidates are all nodes of the other type in id order, and one chain's
// term for (query, candidate) is w = (dS > 700.0) ? 0.0 : exp(-dS) with the ADD dS of the pair (type-a node u, type-b node v)
// the two form: the seven terms of bisbm_edge_probs.hip in their order, bit-equal to what the listed call gives that chain.
//
// IEEE addition commutes, and every two-sided term of dS is (half of u) + (half of v): it is formed here as (the query's half) +
// (the candidate's half) for either query type.  What depends on what, and where it is computed:
//   chain and block, chain, block and degree    `blk` and `etat` of a range of chains: the two term kernels of bisbm_edge_probs.hip
//   chain and cell of the quadrant of m         `tm` of the range: edge_tm_terms_kernel
//   query                                       its half of t_deg and the flags of its present edges: once at the head
//   candidate                                   its degree and its half of t_deg: once at the head
//   chain and query                             its block's halves of t_mr and t_q, its eta half, its row (column, for type-b
//                                               queries) of t_m = lg(m+1) - lg(m+2) over the other type's blocks: staged in LDS
//                                               by the workgroup, two buffers, one barrier per chain.  The t_m row is a copy:
//                                               edge_tm_terms_kernel fills t_m of every cell of the quadrant for the range
//                                               first (thread = (chain, cell)).  Making the row while staging instead -- one
//                                               read of m and two gathers of the lgamma table per entry -- measured 2 to 5 %
//                                               slower
//   chain and candidate                         the label (four of a lane as one word), its block's halves from the LDS copy of
//                                               the other type's rows of `blk`, its eta half: two gathers of `etat` from HBM --
//                                               shared by all queries of the tile
//   chain, query and candidate                  one LDS read of t_m, the adds, one exp, one add onto the cell
// t_mult = lg(mu+2) - lg(mu+1) is +0.0 for mu = 0 and the sum before it is never -0.0 (a difference of equal values is +0.0), so
// a cell that is no present edge skips the add.  A lane finds the present edges among its cells once, by binary search in the
// query's sorted distinct neighbours, and keeps one flag bit per cell; in the chain loop only flagged cells look their t_mult up.
//
// A workgroup owns kEdgeQueryCandTile candidates x kEdgeQueryTile queries of one type (bisbm_cand_lanes.hpp), keeps the 4 x 8
// cells of a lane in registers and walks the counted chains of a range in ascending order, one f64 add per chain onto the cell;
// the ranges of a sample follow each other on the stream, each reading the cells the one before stored.  The bits do not depend
// on tiles, ranges or grids.
#include "bisbm_cand_lanes.hpp"
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256, kRowStride = 256;  // (a type has at most 255 blocks while the labels are bytes)
constexpr uint32_t kT = kEdgeQueryTile;
constexpr size_t kTmTermBytes = (size_t)256 << 20;  // t_m terms of one launch: [chains of the range][ka*kb] doubles
// t_m rows | t_mr halves, t_q halves of the candidates' type | t_mr half, t_q half, eta half of the queries
constexpr uint32_t kOthAt = kT * kRowStride, kOwnAt = kOthAt + 2 * kRowStride, kBufDoubles = kOwnAt + 3 * kT;
static_assert(kT * 4 <= 32, "one flag bit per cell of a lane");

// the first entry of nbr[lo .. hi) that is not below `node`
__device__ __forceinline__ uint64_t lower_bound_nbr(const uint32_t* nbr, uint64_t lo, uint64_t hi, uint32_t node) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (nbr[mid] < node)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// tm[c][cell] = lg(m+1) - lg(m+2) of every cell of the quadrant of m of the chains of the range; thread = (chain, cell)
__global__ __launch_bounds__(256) void edge_tm_terms_kernel(EdgeQueryParams p) {
    const size_t quad = (size_t)p.ka * p.kb;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_range * quad) return;
    if (p.rung && p.rung[p.c0 + i / quad] != 0u) return;  // (not counted: never read)
    const Tables tab{p.lg, p.lg_size, nullptr, 0, nullptr};
    const long long mm = p.m[(size_t)p.c0 * quad + i];
    p.tm[i] = lgamma_fast(tab, mm + 1) - lgamma_fast(tab, mm + 2);
}

template <bool TYPE_B>
__global__ __launch_bounds__(256) void edge_queries_kernel(EdgeQueryParams p) {
    __shared__ double tabs[2][kBufDoubles];
    __shared__ uint32_t q_node[kT], q_deg[kT];
    __shared__ uint64_t q_nbr[kT][2];
    __shared__ double q_tdeg[kT];
    const uint32_t first = TYPE_B ? 0u : p.na, n_other = TYPE_B ? p.na : p.n - p.na;
    const uint32_t k_oth = TYPE_B ? p.ka : p.kb, lab_oth = TYPE_B ? 0u : p.ka, lab_own = TYPE_B ? p.ka : 0u;
    const uint32_t cand_tile = blockIdx.x % p.cand_tiles, q0 = (p.q_tile0 + blockIdx.x / p.cand_tiles) * kT;
    const uint32_t nq = min(kT, p.n_list - q0);
    const uint32_t K = p.ka + p.kb, quad = p.ka * p.kb, D = p.maxdeg + 1;
    const Tables tab{p.lg, p.lg_size, nullptr, 0, nullptr};

    const CandLanes cl = cand_lanes(first, n_other, cand_tile);
    uint32_t dv[4];
    double c_tdeg[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        dv[j] = cl.valid[j] ? p.rowptr[cl.node(j) + 1] - p.rowptr[cl.node(j)] : 0u;
        c_tdeg[j] = lgamma_fast(tab, (long long)dv[j] + 1) - lgamma_fast(tab, (long long)dv[j] + 2);
    }
    if (threadIdx.x < nq) {
        const uint32_t qi = p.list[q0 + threadIdx.x], q = p.queries[qi];
        const uint32_t dq = p.rowptr[q + 1] - p.rowptr[q];
        q_node[threadIdx.x] = q, q_deg[threadIdx.x] = dq;
        q_nbr[threadIdx.x][0] = p.nbr_ptr[qi], q_nbr[threadIdx.x][1] = p.nbr_ptr[qi + 1];
        q_tdeg[threadIdx.x] = lgamma_fast(tab, (long long)dq + 1) - lgamma_fast(tab, (long long)dq + 2);
    }
    double acc[kT][4];
#pragma unroll
    for (uint32_t i = 0; i < kT; ++i) {
        const double* row = i < nq ? p.sum + p.off[p.list[q0 + i]] : nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = (i < nq && cl.valid[j]) ? row[cl.node(j) - first] : 0.;
    }
    __syncthreads();
    // bit 4 i + j: candidate j of the lane is a present edge of query i
    uint32_t present = 0;
#pragma unroll
    for (uint32_t i = 0; i < kT; ++i) {
        if (i >= nq) break;  // (the same for every lane)
        const uint64_t lo = q_nbr[i][0], hi = q_nbr[i][1];
        if (lo == hi) continue;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (!cl.valid[j]) continue;
            const uint64_t at = lower_bound_nbr(p.nbr, lo, hi, (uint32_t)cl.node(j));
            if (at < hi && p.nbr[at] == (uint32_t)cl.node(j)) present |= 1u << (4 * i + j);
        }
    }

    const double gain0 = lgamma_fast(tab, 1) - lgamma_fast(tab, 2);  // the second form of an eta entry beyond max_degree (eta = 0)
    uint32_t buf = 0;
    for (uint32_t cb = 0; cb < p.n_range; ++cb) {
        const uint32_t c = p.c0 + cb;
        if (p.rung && p.rung[c] != 0u) continue;  // (the same for every lane)
        const double* tm_c = p.tm + (size_t)cb * quad;
        const double* blk_c = p.blk + (size_t)cb * K * 4;
        const double* et_c = p.etat + (size_t)cb * K * D * 2;
        const uint8_t* lab = p.labels + (size_t)c * p.label_stride;
        // the buffer the chain before last used: every wave has passed the barrier of the last chain since it read it
        double* t = tabs[buf];
        for (uint32_t i = threadIdx.x; i < nq * k_oth; i += kLanes) {
            const uint32_t qi = i / k_oth, x = i - qi * k_oth, b = (uint32_t)lab[q_node[qi]] - lab_own;
            t[qi * kRowStride + x] = TYPE_B ? tm_c[x * p.kb + b] : tm_c[b * p.kb + x];
        }
        for (uint32_t i = threadIdx.x; i < k_oth; i += kLanes) {
            t[kOthAt + i] = blk_c[(size_t)(lab_oth + i) * 4];
            t[kOthAt + kRowStride + i] = blk_c[(size_t)(lab_oth + i) * 4 + 1];
        }
        if (threadIdx.x < nq) {
            const uint32_t b = lab[q_node[threadIdx.x]], dq = q_deg[threadIdx.x];  // (d_q <= max_degree)
            const double* et = et_c + (size_t)b * D * 2;
            t[kOwnAt + threadIdx.x] = blk_c[(size_t)b * 4];
            t[kOwnAt + kT + threadIdx.x] = blk_c[(size_t)b * 4 + 1];
            t[kOwnAt + 2 * kT + threadIdx.x] = et[2 * dq] + (dq + 1 < D ? et[2 * (dq + 1) + 1] : gain0);
        }
        __syncthreads();
        buf ^= 1u;
        const uint32_t word = cl.any ? *(const uint32_t*)(lab + (size_t)cl.w * 4) : 0u;
        uint32_t bv[4];
        double c_mr[4], c_q[4], c_eta[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            bv[j] = cl.valid[j] ? ((word >> (8 * j)) & 255u) - lab_oth : 0u;
            const double* et = et_c + (size_t)(lab_oth + bv[j]) * D * 2;
            c_mr[j] = t[kOthAt + bv[j]];
            c_q[j] = t[kOthAt + kRowStride + bv[j]];
            c_eta[j] = et[2 * dv[j]] + (dv[j] + 1 < D ? et[2 * (dv[j] + 1) + 1] : gain0);
        }
#pragma unroll
        for (uint32_t i = 0; i < kT; ++i) {
            if (i >= nq) break;  // (the same for every lane)
            const double q_mr = t[kOwnAt + i], q_q = t[kOwnAt + kT + i], q_eta = t[kOwnAt + 2 * kT + i], q_td = q_tdeg[i];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                double dS = q_td + c_tdeg[j];              // t_deg
                dS = dS + t[i * kRowStride + bv[j]];       // + t_m
                dS = dS + (q_mr + c_mr[j]);                // + t_mr
                dS = dS + (q_eta + c_eta[j]);              // + t_eta
                dS = dS + (q_q + c_q[j]);                  // + t_q
                if ((present >> (4 * i + j)) & 1u) {       // + t_mult (+0.0 everywhere else)
                    const uint64_t at = lower_bound_nbr(p.nbr, q_nbr[i][0], q_nbr[i][1], (uint32_t)cl.node(j));
                    dS = dS + p.nbr_tmult[at];
                }
                dS = dS + p.tE;
                acc[i][j] += (dS > 700.0) ? 0.0 : exp(-dS);
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kT; ++i) {
        if (i >= nq) break;
        double* row = p.sum + p.off[p.list[q0 + i]];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (cl.valid[j]) row[cl.node(j) - first] = acc[i][j];
    }
}

}  // namespace

namespace bisbm {

hipError_t launch_edge_queries(const EdgeQueryParams& p_in, hipStream_t stream) {
    EdgeQueryParams p = p_in;
    if (p.n_list == 0) return hipSuccess;
    const uint64_t first = p.type ? 0u : p.na, n_other = p.type ? p.na : p.n - p.na;
    if (n_other == 0) return hipSuccess;
    return for_cand_grids(first, n_other, p.n_list, kEdgeQueryTile, [&](uint32_t cand_tiles, uint32_t q_tile0, dim3 grid) {
        p.cand_tiles = cand_tiles, p.q_tile0 = q_tile0;
        if (p.type)
            hipLaunchKernelGGL(edge_queries_kernel<true>, grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL(edge_queries_kernel<false>, grid, dim3(kLanes), 0, stream, p);
    });
}

hipError_t launch_edge_tm_terms(const EdgeQueryParams& p, hipStream_t stream) {
    const size_t cells = (size_t)p.n_range * p.ka * p.kb;
    hipLaunchKernelGGL(edge_tm_terms_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bisbm

namespace {

const char kNoQueries[] = "no edge queries: call bisbm_edge_queries_set first";

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream
int add_sample(bisbm_engine* h, bisbm_engine* e) {
    EdgeQueryState& s = h->edge_queries;
    const uint32_t K = e->ka + e->kb;
    const size_t eta_cells = (size_t)K * (e->maxdeg + 1);  // per chain
    const size_t quad = (size_t)e->ka * e->kb;
    // chains per launch: what keeps the eta terms under their byte cap (or BISBM_EDGE_RANGE_CHAINS), and the t_m terms under the same
    const uint32_t per = (uint32_t)std::min<size_t>(edge_range_chains(e), std::max<size_t>(kTmTermBytes / (sizeof(double) * quad), 1));
    RESERVE(h, s.d_tm, (size_t)per * quad);
    RESERVE(h, s.d_blk, (size_t)per * K * 4);
    RESERVE(h, s.d_etat, (size_t)per * eta_cells * 2);
    const HostTables& tab = *h->tab;
    const uint64_t E = h->num_edges, cells = (uint64_t)e->ka * e->kb;
    EdgeTermParams t{};
    t.ka = e->ka, t.kb = e->kb, t.maxdeg = e->maxdeg;
    t.m_r = e->d_m_r, t.n_r = e->d_n_r, t.eta = e->d_eta;
    t.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    t.tab = Tables{e->d_lgamma, tab.lg.size(), e->d_q, e->q_stride, e->d_logtab};
    t.blk = s.d_blk.get(), t.etat = s.d_etat.get();
    EdgeQueryParams p{};
    p.n = (uint32_t)h->n, p.na = (uint32_t)h->na;
    p.ka = e->ka, p.kb = e->kb, p.maxdeg = e->maxdeg;
    p.queries = s.d_q.get(), p.off = s.d_off.get();
    p.rowptr = h->d_rowptr;
    p.nbr_ptr = s.d_nbr_ptr.get(), p.nbr = s.d_nbr.get(), p.nbr_tmult = s.d_nbr_tmult.get();
    p.labels = e->d_labels;
    p.label_stride = e->label_stride;
    p.m = e->d_m;
    p.rung = t.rung;
    p.lg = e->d_lgamma, p.lg_size = tab.lg.size();
    // the edge-count prior of this shape (entropy_terms: t[2] = lbinom(ka kb + E - 1, E)), as the listed call forms it
    p.tE = h_lbinom_fast(tab, cells + E, E + 1) - h_lbinom_fast(tab, cells + E - 1, E);
    p.blk = t.blk, p.etat = t.etat;
    p.tm = s.d_tm.get();
    p.sum = s.d_sum.get();
    for (uint32_t c0 = 0; c0 < e->n_chains; c0 += per) {  // (the ranges in ascending order, one after the other on the stream)
        t.c0 = p.c0 = c0, t.n_range = p.n_range = std::min(per, e->n_chains - c0);
        HIPCHK(h, launch_edge_terms(t, h->stream));
        HIPCHK(h, launch_edge_tm_terms(p, h->stream));
        for (uint32_t type = 0; type < 2; ++type) {
            p.type = type;
            p.n_list = type ? s.n - s.n_a : s.n_a;
            p.list = s.d_list.get() + (type ? s.n_a : 0u);
            HIPCHK(h, launch_edge_queries(p, h->stream));
        }
    }
    if (e != h) HIPCHK(h, hipStreamSynchronize(h->stream));  // (the next group sizes and fills d_blk and d_etat anew)
    s.terms += e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    return BISBM_OK;
}

const double* sums_of(bisbm_engine* d) { return d->edge_queries.d_sum.get(); }

// the distinct neighbours of every query, ascending, with their multiplicities: from the CSR on the device of `h`
int read_neighbours(bisbm_engine* h, const std::vector<uint32_t>& q, EdgeQueryState& s) {
    std::vector<uint32_t> rowptr((size_t)h->n + 1), row;
    HIPCHK(h, hipMemcpy(rowptr.data(), h->d_rowptr, sizeof(uint32_t) * rowptr.size(), hipMemcpyDeviceToHost));
    s.nbr_ptr.assign(q.size() + 1, 0);
    s.nbr.clear(), s.mult.clear();
    for (size_t i = 0; i < q.size(); ++i) {
        const uint32_t r0 = rowptr[q[i]], r1 = rowptr[q[i] + 1];
        row.resize(r1 - r0);
        if (r1 > r0) HIPCHK(h, hipMemcpy(row.data(), h->d_col + r0, sizeof(uint32_t) * row.size(), hipMemcpyDeviceToHost));
        std::sort(row.begin(), row.end());
        for (size_t k = 0; k < row.size(); ++k) {
            if (k && row[k] == row[k - 1])
                ++s.mult.back();
            else
                s.nbr.push_back(row[k]), s.mult.push_back(1);
        }
        s.nbr_ptr[i + 1] = s.nbr.size();
    }
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_edge_queries_set(bisbm_handle h, uint32_t n_queries, const uint32_t* queries) {
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
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_edge_queries_set(d, n_queries, queries); });
        h->edge_queries = EdgeQueryState();
        if (rc == BISBM_OK && n_queries) {
            EdgeQueryState &s = h->edge_queries, &d = h->devs[0]->edge_queries;  // (every device holds the same graph)
            s.n = n_queries, s.n_a = n_a, s.q = q, s.off = off;
            s.nbr_ptr = d.nbr_ptr, s.nbr = d.nbr, s.mult = d.mult;
        }
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->edge_queries = EdgeQueryState();  // (the old queries, their sums and buffers go)
    if (n_queries == 0) return BISBM_OK;
    EdgeQueryState& s = h->edge_queries;
    if (int rc = read_neighbours(h, q, s)) {
        h->edge_queries = EdgeQueryState();
        return rc;
    }
    const HostTables& tab = *h->tab;
    std::vector<double> tmult(s.nbr.size());  // (the host's table holds the entries of the device's)
    for (size_t k = 0; k < tmult.size(); ++k) tmult[k] = h_lgamma_fast(tab, (uint64_t)s.mult[k] + 2) - h_lgamma_fast(tab, (uint64_t)s.mult[k] + 1);
    const size_t cells = (size_t)off[n_queries];
    hipError_t e = s.d_sum.reserve(cells);
    if (e != hipSuccess) {
        h->edge_queries = EdgeQueryState();
        return fail(h, BISBM_ERR_HIP, "bisbm_edge_queries_set: %zu bytes of device memory for the sums of %u queries could not be allocated: %s",
                    cells * sizeof(double), n_queries, hipGetErrorString(e));
    }
    e = s.d_q.reserve(n_queries);
    if (e == hipSuccess) e = s.d_off.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = s.d_list.reserve(n_queries);
    if (e == hipSuccess) e = s.d_cand.reserve(n_queries);
    if (e == hipSuccess) e = s.d_nbr_ptr.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = s.d_nbr.reserve(s.nbr.size());
    if (e == hipSuccess) e = s.d_nbr_tmult.reserve(s.nbr.size());
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_q.get(), q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off.get(), off.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_list.get(), list.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_cand.get(), cand.data(), sizeof(TopkCand) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_nbr_ptr.get(), s.nbr_ptr.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && !s.nbr.empty()) e = hipMemcpyAsync(s.d_nbr.get(), s.nbr.data(), sizeof(uint32_t) * s.nbr.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && !s.nbr.empty()) e = hipMemcpyAsync(s.d_nbr_tmult.get(), tmult.data(), sizeof(double) * tmult.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_sum.get(), 0, sizeof(double) * cells, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (the host arrays above live until here)
    if (e != hipSuccess) {
        h->edge_queries = EdgeQueryState();
        return fail(h, BISBM_ERR_HIP, "bisbm_edge_queries_set: %s", hipGetErrorString(e));
    }
    s.n = n_queries, s.n_a = n_a;
    s.q.swap(q), s.off.swap(off);
    return BISBM_OK;
}

int bisbm_edge_queries_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->edge_queries.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED,
                    "edge queries serve byte labels only (at most 256 blocks); bisbm_edge_probs_* serves two-byte labels: list the pairs there");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_edge_queries_accumulate");
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_edge_queries_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_edge_queries_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_edge_queries_reset(d); });
    h->edge_queries.terms = 0;
    if (!h->edge_queries.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->edge_queries.d_sum.get(), 0, sizeof(double) * h->edge_queries.off[h->edge_queries.n], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_edge_queries_get_row(bisbm_handle h, uint32_t query_index, double* w_sum_out, uint32_t* mult_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const EdgeQueryState& s = h->edge_queries;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u queries are set", query_index, s.n);
    if (terms_out) *terms_out = total_terms(h, &bisbm_engine::edge_queries);
    const size_t len = (size_t)(s.off[query_index + 1] - s.off[query_index]);
    if (mult_out) {
        const uint32_t first = s.q[query_index] < h->na ? (uint32_t)h->na : 0u;
        std::fill(mult_out, mult_out + len, 0u);
        for (uint64_t k = s.nbr_ptr[query_index]; k < s.nbr_ptr[query_index + 1]; ++k) mult_out[s.nbr[k] - first] = s.mult[k];
    }
    if (!w_sum_out) return BISBM_OK;
    return read_row(h, per_device(h, sums_of), s.off[query_index], len, w_sum_out);
}

int bisbm_edge_queries_topk(bisbm_handle h, uint32_t k, int exclude_neighbours, uint32_t* node_out, double* w_sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const EdgeQueryState& s = h->edge_queries;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_edge_queries_topk selects at most %u candidates per query", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h, &bisbm_engine::edge_queries);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_edge_queries_accumulate before bisbm_edge_queries_topk");
    if (terms_out) *terms_out = terms;
    bisbm_engine* e = device_entries(h)[0];  // the device that selects
    EdgeQueryState& w = e->edge_queries;
    const TopkMaskLists neighbours{e->d_rowptr, nullptr, w.d_q.get(), e->d_col};  // a query's CSR row
    return topk_select(h, __func__, per_device(h, sums_of), s.off, w.topk, w.d_off.get(), w.d_cand.get(), exclude_neighbours ? &neighbours : nullptr, k,
                       node_out, w_sum_out);
}

}  // extern "C"
