// bisbm_foldin.hip -- fold-in queries: a node that is NOT in the graph, given by its type and a list of neighbours of the other
// type, gets a block posterior per chain by the naive-Bayes rule the engine draws its proposals with, and from it an expected
// edge count to every node of the other type (recommend rows) and a soft co-assignment with every node of its own type (similar
// rows), pooled over the chains; the best k of a row are selected on the device by bisbm_topk.hip (no reference counterpart;
// include/bisbm.h, "Fold-in queries", states every f64 operation and its order: a sequential host loop gives the same bits).
//
// Table kernel: one workgroup per (chain, virtual node), lane <-> block.  The factor loop runs over the list in list order
// inside every lane (the order is part of the definition), the neighbours' labels gathered 256 at a time into LDS.  The chain's
// quadrant of m is read through L1 / L2, not staged: a workgroup needs d columns (rows, for a type-b node) of it for the weights
// and one pass over it for the table, the 64 KiB it can reach are shared by all the virtual nodes of the chain, whose
// workgroups are neighbours in the grid, and 64 KiB of LDS per workgroup would leave two workgroups per CU.  The max, Z and the
// table's sums keep their ascending-block order: Z is added by one lane, every lane adds its own table entry.
//
// Rows kernel: the shape of query_scores_kernel.  A workgroup owns kFoldinCandTile candidates x kFoldinTile virtual nodes of one
// type and row kind (bisbm_cand_lanes.hpp), keeps the running sums in registers and walks the chains of the launch in ascending
// order: per chain the tile's table rows (g or P, at most 255 doubles each) go to LDS (two buffers: one barrier per chain), a cell
// is one LDS lookup, for a recommend row one multiply, and one f64 add.
//
// Top-k: the selection of bisbm_topk.hip on the bit patterns of the sums, one table of first candidates per row kind; with the
// listed nodes left out, a virtual node's list is the list that masks.
#include <climits>

#include "bisbm_cand_lanes.hpp"
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256, kRowStride = 256;  // (a type has at most 255 blocks while the labels are bytes)
constexpr size_t kTableBudget = 256ull << 20;      // bytes of recommend tables of one chunk of chains (at least one chain)

__global__ __launch_bounds__(256) void foldin_table_kernel(FoldinTableParams p) {
    __shared__ double s_w[kRowStride], s_P[kRowStride], s_mr[kRowStride];
    __shared__ int s_ex[kRowStride];
    __shared__ uint8_t s_lab[kLanes];
    __shared__ double s_Z;
    __shared__ int s_E;
    const uint32_t tid = threadIdx.x;
    const uint32_t cl = blockIdx.x / p.n_q, slot = blockIdx.x - cl * p.n_q, c = p.chain0 + cl;
    const bool tb = slot >= p.n_a;
    const uint32_t n_b = p.n_q - p.n_a, K = p.ka + p.kb;
    const uint32_t k_own = tb ? p.kb : p.ka, k_oth = tb ? p.ka : p.kb, own0 = tb ? p.ka : 0u, oth0 = tb ? 0u : p.ka;
    double* P = p.P + (size_t)c * ((size_t)p.n_a * p.ka + (size_t)n_b * p.kb) +
                (tb ? (size_t)p.n_a * p.ka + (size_t)(slot - p.n_a) * p.kb : (size_t)slot * p.ka);
    if (p.rung && p.rung[c] != 0u) {  // (the same for every lane) not counted: a NaN row
        if (tid < k_own) P[tid] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const uint32_t qi = p.order[slot];
    const uint64_t l0 = p.ptr[qi], d = p.ptr[qi + 1] - l0;
    const int32_t* m_g = p.m + (size_t)c * p.ka * p.kb;
    const int32_t* mr_g = p.m_r + (size_t)c * K;
    const uint8_t* lab = p.labels + (size_t)c * p.label_stride;

    // 1. block weights as (mantissa, exponent): lane r walks the list in list order
    const bool own = tid < k_own;
    const int32_t nr = own ? p.n_r[(size_t)c * K + own0 + tid] : 0, mr = own ? mr_g[own0 + tid] : 0;
    const bool live = nr > 0;
    int ex = 0;
    double mant = live ? frexp((double)nr, &ex) : 0.;
    const double den = (double)mr + p.alpha * (double)k_oth;
    for (uint64_t j0 = 0; j0 < d; j0 += kLanes) {
        const uint32_t len = (uint32_t)min((uint64_t)kLanes, d - j0);
        __syncthreads();  // (the tile before is read)
        if (tid < len) s_lab[tid] = (uint8_t)((uint32_t)lab[p.nbr[l0 + j0 + tid]] - oth0);
        __syncthreads();
        if (live)
            for (uint32_t j = 0; j < len; ++j) {
                const uint32_t s = s_lab[j];
                const int32_t mm = tb ? m_g[s * p.kb + tid] : m_g[tid * p.kb + s];
                const double x = ((double)mm + p.alpha) / den;
                int e2;
                mant = mant * x;
                mant = frexp(mant, &e2);
                ex += e2;
            }
    }
    // 2. posterior: the largest exponent, the weights scaled by it, Z added in ascending block order by one lane
    s_ex[tid] = live ? ex : INT_MIN;
    s_mr[tid] = (double)mr;
    __syncthreads();
    if (tid == 0) {
        int E = INT_MIN;
        for (uint32_t r = 0; r < k_own; ++r) E = max(E, s_ex[r]);
        s_E = E;
    }
    __syncthreads();
    const int rel = live ? ex - s_E : 0;
    const double w = (!live || rel < -1000) ? 0. : ldexp(mant, rel);
    s_w[tid] = w;
    __syncthreads();
    if (tid == 0) {
        double Z = s_w[0];
        for (uint32_t r = 1; r < k_own; ++r) Z = Z + s_w[r];
        s_Z = Z;
    }
    __syncthreads();
    const double Pr = w / s_Z;
    s_P[tid] = Pr;
    if (own) P[tid] = Pr;
    if (!p.recommend) return;
    __syncthreads();
    // 3. recommend table: lane s adds its entry over the blocks r in ascending order
    if (tid < k_oth) {
        double acc = 0.;
        for (uint32_t r = 0; r < k_own; ++r) {
            const double pr = s_P[r], mrr = s_mr[r];
            if (mrr == 0. || pr == 0.) continue;
            const int32_t mm = tb ? m_g[tid * p.kb + r] : m_g[r * p.kb + tid];
            acc = acc + (pr * (double)mm) / mrr;
        }
        const int32_t mro = mr_g[oth0 + tid];
        double* g = p.g + (size_t)cl * ((size_t)p.n_a * p.kb + (size_t)n_b * p.ka) +
                    (tb ? (size_t)p.n_a * p.kb + (size_t)(slot - p.n_a) * p.ka : (size_t)slot * p.kb);
        g[tid] = mro == 0 ? 0. : acc / (double)mro;
    }
}

template <bool REC>
__global__ __launch_bounds__(256) void foldin_rows_kernel(FoldinRowsParams p) {
    __shared__ double tabs[2][kFoldinTile * kRowStride];
    __shared__ double q_deg[kFoldinTile];
    const uint32_t cand_tile = blockIdx.x % p.cand_tiles, q0 = (p.q_tile0 + blockIdx.x / p.cand_tiles) * kFoldinTile;
    const uint32_t nq = min(kFoldinTile, p.n_list - q0);

    const CandLanes cl = cand_lanes(p.first, p.n_cand, cand_tile);
    double dv[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) dv[j] = (REC && cl.valid[j]) ? (double)(p.rowptr[cl.node(j) + 1] - p.rowptr[cl.node(j)]) : 0.;
    if (threadIdx.x < nq) {
        const uint32_t qi = p.order[p.slot0 + q0 + threadIdx.x];
        q_deg[threadIdx.x] = (double)(p.ptr[qi + 1] - p.ptr[qi]);
    }
    double acc[kFoldinTile][4];
#pragma unroll
    for (uint32_t i = 0; i < kFoldinTile; ++i) {
        const double* row = i < nq ? p.sum + p.off[p.order[p.slot0 + q0 + i]] : nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = (i < nq && cl.valid[j]) ? row[cl.node(j) - p.first] : 0.;
    }
    __syncthreads();

    uint32_t buf = 0;
    for (uint32_t c = 0; c < p.n_chains; ++c) {
        if (p.rung && p.rung[p.chain0 + c] != 0u) continue;  // (the same for every lane)
        const double* src = p.tab + (size_t)c * p.chain_stride + p.type_base + (size_t)q0 * p.k_tab;  // the tile's rows, back to back
        const uint8_t* lab = p.labels + (size_t)(p.chain0 + c) * p.label_stride;
        // the buffer the chain before last used: every wave has passed the barrier of the last chain since it read it
        double* t = tabs[buf];
        for (uint32_t i = threadIdx.x; i < nq * p.k_tab; i += kLanes) {
            const uint32_t qi = i / p.k_tab, x = i - qi * p.k_tab;
            t[qi * kRowStride + x] = src[i];
        }
        __syncthreads();
        buf ^= 1u;
        const uint32_t word = cl.any ? *(const uint32_t*)(lab + (size_t)cl.w * 4) : 0u;
        uint32_t bv[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) bv[j] = cl.valid[j] ? ((word >> (8 * j)) & 255u) - p.lab0 : 0u;
#pragma unroll
        for (uint32_t i = 0; i < kFoldinTile; ++i) {
            if (i >= nq) break;  // (the same for every lane)
            const double dq = q_deg[i];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const double x = t[i * kRowStride + bv[j]];
                // (a candidate of degree 0 adds (d_q * 0.0) * g = +0.0: the sum keeps its bits)
                acc[i][j] += REC ? (dq * dv[j]) * x : x;
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kFoldinTile; ++i) {
        if (i >= nq) break;
        double* row = p.sum + p.off[p.order[p.slot0 + q0 + i]];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (cl.valid[j]) row[cl.node(j) - p.first] = acc[i][j];
    }
}

}  // namespace

namespace bisbm {

hipError_t launch_foldin_tables(const FoldinTableParams& p, hipStream_t stream) {
    if (p.n_q == 0 || p.n_chains == 0) return hipSuccess;
    hipLaunchKernelGGL(foldin_table_kernel, dim3(p.n_chains * p.n_q), dim3(kLanes), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_foldin_rows(const FoldinRowsParams& p_in, bool recommend, hipStream_t stream) {
    FoldinRowsParams p = p_in;
    if (p.n_list == 0 || p.n_cand == 0 || p.n_chains == 0) return hipSuccess;
    return for_cand_grids(p.first, p.n_cand, p.n_list, kFoldinTile, [&](uint32_t cand_tiles, uint32_t q_tile0, dim3 grid) {
        p.cand_tiles = cand_tiles, p.q_tile0 = q_tile0;
        if (recommend)
            hipLaunchKernelGGL(foldin_rows_kernel<true>, grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL(foldin_rows_kernel<false>, grid, dim3(kLanes), 0, stream, p);
    });
}

}  // namespace bisbm

namespace {

constexpr uint32_t kKinds = BISBM_FOLDIN_RECOMMEND | BISBM_FOLDIN_SIMILAR;

const char* kNoQueries = "no virtual nodes: call bisbm_foldin_set first";

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream; the
// posteriors go to segment `seg` of h's d_P
int add_sample(bisbm_engine* h, bisbm_engine* e, const FoldinState::Segment& seg) {
    FoldinState& s = h->foldin;
    const uint32_t n_b = s.n - s.n_a;
    const size_t g_chain = (size_t)s.n_a * e->kb + (size_t)n_b * e->ka, p_chain = (size_t)s.n_a * e->ka + (size_t)n_b * e->kb;
    const bool rec = (s.what & BISBM_FOLDIN_RECOMMEND) != 0, sim = (s.what & BISBM_FOLDIN_SIMILAR) != 0;
    // the chains of one launch: what the budget of the recommend tables holds, and what a one-dimensional grid of (chain, node) does
    uint32_t chunk = std::max<uint32_t>(1u, (1u << 30) / s.n);
    if (rec) chunk = (uint32_t)std::min<uint64_t>(chunk, std::max<uint64_t>(1, kTableBudget / (g_chain * sizeof(double))));
    chunk = std::min(chunk, e->n_chains);
    if (rec) RESERVE(h, s.d_g, (size_t)chunk * g_chain);
    const uint32_t* rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    FoldinTableParams t{};
    t.na = (uint32_t)h->na, t.ka = e->ka, t.kb = e->kb;
    t.n_q = s.n, t.n_a = s.n_a, t.recommend = rec ? 1u : 0u, t.alpha = s.alpha;
    t.order = s.d_order.get(), t.ptr = s.d_ptr.get(), t.nbr = s.d_nbr.get();
    t.labels = e->d_labels, t.label_stride = e->label_stride;
    t.m = e->d_m, t.m_r = e->d_m_r, t.n_r = e->d_n_r, t.rung = rung;
    t.P = s.d_P.get() + seg.base, t.g = s.d_g.get();
    FoldinRowsParams r{};
    r.order = s.d_order.get(), r.ptr = s.d_ptr.get();
    r.rowptr = h->d_rowptr, r.labels = e->d_labels, r.label_stride = e->label_stride, r.rung = rung;
    for (uint32_t c0 = 0; c0 < e->n_chains; c0 += chunk) {
        t.chain0 = r.chain0 = c0;
        t.n_chains = r.n_chains = std::min(chunk, e->n_chains - c0);
        HIPCHK(h, launch_foldin_tables(t, h->stream));
        for (uint32_t type = 0; type < 2; ++type) {
            r.slot0 = type ? s.n_a : 0u, r.n_list = type ? n_b : s.n_a;
            if (rec) {  // candidates: the other type; the table is g
                r.first = type ? 0u : (uint32_t)h->na, r.n_cand = (uint32_t)(type ? h->na : h->nb);
                r.lab0 = type ? 0u : e->ka, r.k_tab = type ? e->ka : e->kb;
                r.tab = s.d_g.get(), r.chain_stride = g_chain, r.type_base = type ? (size_t)s.n_a * e->kb : 0;
                r.off = s.d_off[0].get(), r.sum = s.d_sum[0].get();
                HIPCHK(h, launch_foldin_rows(r, true, h->stream));
            }
            if (sim) {  // candidates: the own type; the table is P
                r.first = type ? (uint32_t)h->na : 0u, r.n_cand = (uint32_t)(type ? h->nb : h->na);
                r.lab0 = type ? e->ka : 0u, r.k_tab = type ? e->kb : e->ka;
                r.tab = s.d_P.get() + seg.base + (size_t)c0 * p_chain, r.chain_stride = p_chain, r.type_base = type ? (size_t)s.n_a * e->ka : 0;
                r.off = s.d_off[1].get(), r.sum = s.d_sum[1].get();
                HIPCHK(h, launch_foldin_rows(r, false, h->stream));
            }
        }
    }
    s.terms += e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    return BISBM_OK;
}

// every device entry's rows of one kind
std::vector<const double*> sums_of(bisbm_engine* h, int kind) {
    return per_device(h, [kind](bisbm_engine* d) { return (const double*)d->foldin.d_sum[kind].get(); });
}

// which of the two row kinds `what` names: 0 recommend, 1 similar; refusals as BISBM_ERR_INVALID_ARG
int kind_of(bisbm_engine* h, uint32_t what, int* kind) {
    if (what != BISBM_FOLDIN_RECOMMEND && what != BISBM_FOLDIN_SIMILAR)
        return fail(h, BISBM_ERR_INVALID_ARG, "what = %u: exactly one of BISBM_FOLDIN_RECOMMEND and BISBM_FOLDIN_SIMILAR", what);
    if (!(h->foldin.what & what))
        return fail(h, BISBM_ERR_INVALID_ARG, "the %s rows are not kept: bisbm_foldin_set was called without that bit of `what`",
                    what == BISBM_FOLDIN_RECOMMEND ? "recommend" : "similar");
    *kind = what == BISBM_FOLDIN_RECOMMEND ? 0 : 1;
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_foldin_set(bisbm_handle h, uint32_t n_queries, const uint8_t* type, const uint64_t* list_ptr, const uint32_t* list, double alpha,
                     uint32_t what) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    FoldinState f;
    if (n_queries) {  // (before anything changes: a refused call leaves the earlier virtual nodes in place)
        if (!type || !list_ptr || !list) return fail(h, BISBM_ERR_INVALID_ARG, "type, list_ptr or list is NULL");
        if (!(alpha > 0.) || !std::isfinite(alpha)) return fail(h, BISBM_ERR_INVALID_ARG, "alpha = %g: a finite value above 0 is needed", alpha);
        if (what == 0 || (what & ~kKinds)) return fail(h, BISBM_ERR_INVALID_ARG, "what = %u: a mask of BISBM_FOLDIN_RECOMMEND (1) and BISBM_FOLDIN_SIMILAR (2)", what);
        if (list_ptr[0] != 0) return fail(h, BISBM_ERR_INVALID_ARG, "list_ptr[0] = %llu: must be 0", (unsigned long long)list_ptr[0]);
        for (uint32_t i = 0; i < n_queries; ++i) {
            if (type[i] > 1) return fail(h, BISBM_ERR_INVALID_ARG, "query %u: type %u is neither 0 (a) nor 1 (b)", i, type[i]);
            if (list_ptr[i + 1] <= list_ptr[i]) return fail(h, BISBM_ERR_INVALID_ARG, "query %u: an empty list (a virtual node needs at least one neighbour)", i);
            for (uint64_t j = list_ptr[i]; j < list_ptr[i + 1]; ++j) {
                const bool ok = type[i] ? list[j] < h->na : (list[j] >= h->na && list[j] < h->n);
                if (!ok)
                    return fail(h, BISBM_ERR_INVALID_ARG, "query %u position %llu: %u is not a node of type %c", i,
                                (unsigned long long)(j - list_ptr[i]), list[j], type[i] ? 'a' : 'b');
            }
        }
        f.n = n_queries, f.what = what, f.alpha = alpha;
        f.type.assign(type, type + n_queries);
        f.ptr.assign(list_ptr, list_ptr + n_queries + 1);
        f.list.assign(list, list + list_ptr[n_queries]);
        f.slot.resize(n_queries);
        for (uint32_t i = 0; i < n_queries; ++i) f.n_a += type[i] == 0;
        for (int kind = 0; kind < 2; ++kind) {
            f.off[kind].assign((size_t)n_queries + 1, 0);
            if (what & (1u << kind))
                for (uint32_t i = 0; i < n_queries; ++i) {  // recommend: the other type's nodes; similar: the own type's
                    const bool cand_b = (type[i] != 0) == (kind == 1);  // (a type-a node's recommend row, a type-b node's similar row)
                    f.off[kind][i + 1] = f.off[kind][i] + (cand_b ? h->nb : h->na);
                }
        }
    }
    if (!h->devs.empty()) {
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_foldin_set(d, n_queries, type, list_ptr, list, alpha, what); });
        h->foldin = FoldinState();
        if (rc == BISBM_OK && n_queries) h->foldin = std::move(f);
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->foldin = FoldinState();  // (the old virtual nodes, their sums and buffers go)
    if (n_queries == 0) return BISBM_OK;
    std::vector<uint32_t> order(n_queries);
    uint32_t at_a = 0, at_b = f.n_a;
    for (uint32_t i = 0; i < n_queries; ++i) {
        f.slot[i] = type[i] ? at_b++ : at_a++;
        order[f.slot[i]] = i;
    }
    std::vector<TopkCand> cand[2];  // a row's first candidate, every candidate eligible: type b's first node where `off` counted nb
    for (int kind = 0; kind < 2; ++kind)
        for (uint32_t i = 0; i < n_queries; ++i) cand[kind].push_back(TopkCand{(type[i] != 0) == (kind == 1) ? (uint32_t)h->na : 0u, 0xffffffffu});
    hipError_t e = hipSuccess;
    for (int kind = 0; kind < 2 && e == hipSuccess; ++kind) {
        const size_t cells = (size_t)f.off[kind][n_queries];
        if (!cells) continue;
        e = f.d_sum[kind].reserve(cells);
        if (e != hipSuccess)
            return fail(h, BISBM_ERR_HIP, "bisbm_foldin_set: %zu bytes of device memory for the %s rows of %u virtual nodes could not be allocated: %s",
                        cells * sizeof(double), kind ? "similar" : "recommend", n_queries, hipGetErrorString(e));
        e = hipMemsetAsync(f.d_sum[kind].get(), 0, sizeof(double) * cells, h->stream);
    }
    if (e == hipSuccess) e = f.d_ptr.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = f.d_nbr.reserve(f.list.size());
    if (e == hipSuccess) e = f.d_order.reserve(n_queries);
    if (e == hipSuccess) e = f.d_off[0].reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = f.d_off[1].reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(f.d_ptr.get(), f.ptr.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.d_nbr.get(), f.list.data(), sizeof(uint32_t) * f.list.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.d_order.get(), order.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    for (int kind = 0; kind < 2; ++kind) {
        if (e == hipSuccess) e = f.d_cand[kind].reserve(n_queries);
        if (e == hipSuccess)
            e = hipMemcpyAsync(f.d_off[kind].get(), f.off[kind].data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(f.d_cand[kind].get(), cand[kind].data(), sizeof(TopkCand) * n_queries, hipMemcpyHostToDevice, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (`order`, `cand` and f's vectors are read until here)
    if (e != hipSuccess) return fail(h, BISBM_ERR_HIP, "bisbm_foldin_set: %s", hipGetErrorString(e));
    h->foldin = std::move(f);
    return BISBM_OK;
}

int bisbm_foldin_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->foldin.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "fold-in queries serve byte labels only (at most 256 blocks): merge the blocks down first");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_foldin_accumulate");
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_foldin_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    FoldinState& s = h->foldin;
    // the posteriors of this sample: one segment per leaf, chains in the leaf's order
    s.segments.clear();
    size_t total = 0;
    for (bisbm_engine* e : leaves(h)) {
        FoldinState::Segment seg;
        seg.ka = e->ka, seg.kb = e->kb, seg.base = total;
        seg.chain.resize(e->n_chains);
        for (uint32_t c = 0; c < e->n_chains; ++c) seg.chain[c] = e == h ? c : e->ridx[c];
        total += (size_t)e->n_chains * ((size_t)s.n_a * e->ka + (size_t)(s.n - s.n_a) * e->kb);
        s.segments.push_back(std::move(seg));
    }
    hipError_t err = s.d_P.reserve(total);
    if (err != hipSuccess) {
        s.segments.clear();
        return fail(h, BISBM_ERR_HIP, "bisbm_foldin_accumulate: %zu bytes of device memory for the posteriors of one sample could not be allocated: %s",
                    total * sizeof(double), hipGetErrorString(err));
    }
    size_t i = 0;
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e, s.segments[i++])) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_foldin_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_foldin_reset(d); });
    FoldinState& s = h->foldin;
    s.terms = 0;
    s.segments.clear();
    if (!s.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    for (int kind = 0; kind < 2; ++kind)
        if (s.off[kind][s.n]) HIPCHK(h, hipMemsetAsync(s.d_sum[kind].get(), 0, sizeof(double) * s.off[kind][s.n], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_foldin_get_posteriors(bisbm_handle h, uint32_t query_index, uint32_t stride, double* p_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const FoldinState& s = h->foldin;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u virtual nodes are set", query_index, s.n);
    if (!p_out) return fail(h, BISBM_ERR_INVALID_ARG, "p_out is NULL");
    const std::vector<bisbm_engine*> entries = device_entries(h);
    const bool tb = s.type[query_index] != 0;
    for (bisbm_engine* d : entries) {
        if (d->foldin.segments.empty()) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_foldin_accumulate before bisbm_foldin_get_posteriors");
        for (const FoldinState::Segment& seg : d->foldin.segments)
            if (stride < (tb ? seg.kb : seg.ka))
                return fail(h, BISBM_ERR_INVALID_ARG, "stride = %u: a chain has %u blocks of the virtual node's type", stride, tb ? seg.kb : seg.ka);
    }
    DeviceGuard keep;
    std::vector<double> tmp;
    for (size_t di = 0; di < entries.size(); ++di) {
        bisbm_engine* d = entries[di];
        const FoldinState& ds = d->foldin;
        const uint32_t chain_base = h->devs.empty() ? 0u : h->dev_first[di], slot = ds.slot[query_index], n_b = ds.n - ds.n_a;
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        for (const FoldinState::Segment& seg : ds.segments) {
            const size_t k_own = tb ? seg.kb : seg.ka, p_chain = (size_t)ds.n_a * seg.ka + (size_t)n_b * seg.kb;
            const size_t at = tb ? (size_t)ds.n_a * seg.ka + (size_t)(slot - ds.n_a) * seg.kb : (size_t)slot * seg.ka;
            tmp.resize(seg.chain.size() * k_own);
            HIPCHK(h, hipMemcpy2D(tmp.data(), k_own * sizeof(double), ds.d_P.get() + seg.base + at, p_chain * sizeof(double), k_own * sizeof(double),
                                  seg.chain.size(), hipMemcpyDeviceToHost));
            for (size_t c = 0; c < seg.chain.size(); ++c) {
                double* row = p_out + (size_t)(chain_base + seg.chain[c]) * stride;
                const bool counted = !std::isnan(tmp[c * k_own]);
                for (size_t x = 0; x < stride; ++x)  // (a chain that was not counted: NaN over the whole row)
                    row[x] = !counted ? std::numeric_limits<double>::quiet_NaN() : x < k_own ? tmp[c * k_own + x] : 0.;
            }
        }
    }
    return BISBM_OK;
}

int bisbm_foldin_get_row(bisbm_handle h, uint32_t what, uint32_t query_index, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const FoldinState& s = h->foldin;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    int kind = 0;
    if (int rc = kind_of(h, what, &kind)) return rc;
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u virtual nodes are set", query_index, s.n);
    if (terms_out) *terms_out = total_terms(h, &bisbm_engine::foldin);
    if (!sum_out) return BISBM_OK;
    const std::vector<uint64_t>& off = s.off[kind];
    return read_row(h, sums_of(h, kind), off[query_index], (size_t)(off[query_index + 1] - off[query_index]), sum_out);
}

int bisbm_foldin_topk(bisbm_handle h, uint32_t what, uint32_t k, int exclude_listed, uint32_t* node_out, double* sum_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const FoldinState& s = h->foldin;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    int kind = 0;
    if (int rc = kind_of(h, what, &kind)) return rc;
    if (exclude_listed && kind == 1)
        return fail(h, BISBM_ERR_INVALID_ARG, "exclude_listed with the similar rows: a virtual node has no node of its own type to leave out");
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_foldin_topk selects at most %u candidates per virtual node", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h, &bisbm_engine::foldin);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_foldin_accumulate before bisbm_foldin_topk");
    if (terms_out) *terms_out = terms;
    FoldinState& w = device_entries(h)[0]->foldin;  // the device that selects
    const TopkMaskLists listed{nullptr, w.d_ptr.get(), nullptr, w.d_nbr.get()};  // a virtual node's list
    return topk_select(h, __func__, sums_of(h, kind), s.off[kind], w.topk, w.d_off[kind].get(), w.d_cand[kind].get(), exclude_listed ? &listed : nullptr,
                       k, node_out, sum_out);
}

}  // extern "C"
