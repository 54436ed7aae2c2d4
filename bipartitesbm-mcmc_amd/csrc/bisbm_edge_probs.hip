// bisbm_edge_probs.hip -- exact edge probabilities pooled over chains (no reference counterpart: the reference keeps one graph).
// For a listed pair (u, v, kind), u of type a and v of type b, one chain contributes
//     dS = S(G + e, b) - S(G, b)  (kind ADD)   or   S(G - e, b) - S(G, b)  (kind REMOVE),
// the change of the full description length (blockmodel.cc:753-787) when one edge (u, v) is added to or taken from the graph
// while the partition stays: seven terms in a fixed order, spelled out in include/bisbm.h ("Edge probabilities").  A sample adds
// dS and w = exp(-dS) of every counted chain to the pair's two running f64 sums, chain by chain in ascending order.
//
// What depends on what, and where it is computed:
//   pair only          d_u, d_v, the multiplicity mu, t_deg, t_mult    once at `set`, edge_pairs_kernel (mu: a scan of the
//                                                                      shorter of the two CSR rows)
//   launch only        t_E (one value for ADD, one for REMOVE)         on the host from the host's lgamma table (the same
//                                                                      entries the device holds), a kernel argument
//   chain and block    the halves of t_mr and t_q: for block x         edge_block_terms_kernel: thread = (chain, block),
//                      lg(m_r+2) - lg(m_r+1), logq(m_r+1) - logq(m_r)  K x 3 log_q per chain instead of 4 per (pair, chain);
//                      and their REMOVE forms                          t_mr and t_q are each (half of r) + (half of s), so the
//                                                                      sums carry the same bits as the expressions written out
//   chain, block and   the two forms an eta entry takes in t_eta:       edge_eta_terms_kernel: thread = (chain, block, degree);
//   degree             lg(eta+1) - lg(eta) (the entry that loses a      t_eta is ((first of [r][d_u] + second of [r][d_u +- 1])
//                      node), lg(eta+1) - lg(eta+2) (the one that       + (... of s)): four gathers of a double per (pair,
//                      gains one)                                       chain) instead of four of eta and eight of lgamma
//   pair and chain     t_m (m[r][s]), the sums                          edge_probs_kernel
//
// Tiling: a launch serves a RANGE of consecutive chains of one engine -- all of them while their eta terms stay below
// kEtaTermBytes, the ranges in ascending order otherwise.  The two small kernels first fill the block terms and the eta terms of
// the range.  edge_probs_kernel then runs one workgroup per tile of kEdgeProbsTile pairs (4 per lane: the pair's constants and
// its two running sums stay in registers) and walks the chains of the range in ascending order: per counted chain it stages the
// chain's block terms and its quadrant of m in LDS (byte labels; two buffers, so one barrier per chain; a wide handle reads both
// from HBM), then every lane takes its pairs: label gather, LDS lookups, four gathers of eta terms from HBM, two of the lgamma
// table (t_m), dS, exp, two adds.  The sums are read once before the first chain of the range and stored once after its last,
// so a pair's sums see its chains one at a time in ascending chain index whatever the tile or the grid -- no partial sums, no
// floating-point atomics, and a sequential host loop gives the same bits.  With BISBM_EDGE_KEEP_LAST every dS is also stored to
// the chain's row of `last` (NaN for a chain that is not counted).  The pairs are held sorted by (u, v), so the b_u gather of a
// tile walks a short stretch of the label array.
//
// The edge queries (bisbm_edge_queries.hip) take the block terms and the eta terms of a range from the same two kernels
// (launch_edge_terms) and size their ranges by the same rule (edge_range_chains).
#include "bisbm_device.hpp"
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256, kPerLane = kEdgeProbsTile / kLanes;
constexpr size_t kEtaTermBytes = (size_t)256 << 20;  // eta terms of one launch: [chains of the range][K][maxdeg + 1][2] doubles

struct EdgePairParams {
    uint32_t n_pairs;
    const uint32_t *rowptr, *col, *u, *v;
    const uint8_t* kind;
    const double* lg;
    uint64_t lg_size;
    uint32_t *du, *dv, *mult;
    double *tdeg, *tmult;
};

struct EdgeProbParams {
    uint32_t n_pairs, ka, kb, maxdeg, c0, n_range;  // chains c0 .. c0 + n_range - 1 of the engine
    const uint32_t *u, *v, *du, *dv;
    const uint8_t* kind;
    const double *tdeg, *tmult;
    const uint8_t* labels;
    size_t label_stride;
    const int32_t *m, *m_r, *n_r;  // [chain][ka*kb], [chain][K], [chain][K]
    const uint32_t* eta;           // [chain][K][maxdeg + 1]
    const uint32_t* rung;          // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    Tables tab;
    double tE[2];                  // t_E of ADD, of REMOVE
    double* blk;                   // [n_range][K][4] block terms: {t_mr half, t_q half} of ADD, of REMOVE
    double* etat;                  // [n_range][K][maxdeg + 1][2] eta terms: {lg(eta+1) - lg(eta), lg(eta+1) - lg(eta+2)}
    double *dS_sum, *w_sum;        // [n_pairs] running sums
    double* last;                  // KEEP_LAST: [rows][n_pairs] dS of this sample; NULL: not kept
    const uint32_t* row;           // row of `last` of every chain; NULL: the chain's index
};

// d_u, d_v, mu, t_deg, t_mult of every pair
__global__ __launch_bounds__(256) void edge_pairs_kernel(EdgePairParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_pairs) return;
    const Tables tab{p.lg, p.lg_size, nullptr, 0, nullptr};
    const uint32_t a = p.u[i], b = p.v[i];
    const uint32_t a0 = p.rowptr[a], a1 = p.rowptr[a + 1], b0 = p.rowptr[b], b1 = p.rowptr[b + 1];
    const uint32_t da = a1 - a0, db = b1 - b0;
    uint32_t mu = 0;
    if (da <= db) {
        for (uint32_t k = a0; k < a1; ++k) mu += p.col[k] == b;
    } else {
        for (uint32_t k = b0; k < b1; ++k) mu += p.col[k] == a;
    }
    p.du[i] = da, p.dv[i] = db, p.mult[i] = mu;
    // (a REMOVE of an edge that is not there reads lg(0) = +inf here: `set` refuses the call once it has the multiplicities)
    const long long d2 = p.kind[i] == BISBM_EDGE_REMOVE ? 0 : 2;
    p.tdeg[i] = (lgamma_fast(tab, (long long)da + 1) - lgamma_fast(tab, (long long)da + d2)) +
                (lgamma_fast(tab, (long long)db + 1) - lgamma_fast(tab, (long long)db + d2));
    p.tmult[i] = d2 ? lgamma_fast(tab, (long long)mu + 2) - lgamma_fast(tab, (long long)mu + 1)
                    : lgamma_fast(tab, (long long)mu) - lgamma_fast(tab, (long long)mu + 1);
}

// blk[c][x] = {lg(m_r+2) - lg(m_r+1), logq(m_r+1, n_r) - logq(m_r, n_r), lg(m_r) - lg(m_r+1), logq(m_r-1, n_r) - logq(m_r, n_r)}
// with the log_q of the entropy kernel (log_q<false>, its argument order); thread = (chain, block)
__global__ __launch_bounds__(256) void edge_block_terms_kernel(EdgeProbParams p) {
    const uint32_t K = p.ka + p.kb;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_range * K) return;
    if (p.rung && p.rung[p.c0 + i / K] != 0u) return;  // (not counted: never read)
    const int mr = p.m_r[(size_t)p.c0 * K + i], nr = p.n_r[(size_t)p.c0 * K + i];
    const double q0 = log_q<false>(p.tab, mr, nr);
    double* o = p.blk + (size_t)i * 4;
    o[0] = lgamma_fast(p.tab, (long long)mr + 2) - lgamma_fast(p.tab, (long long)mr + 1);
    o[1] = log_q<false>(p.tab, mr + 1, nr) - q0;
    o[2] = lgamma_fast(p.tab, (long long)mr) - lgamma_fast(p.tab, (long long)mr + 1);
    o[3] = log_q<false>(p.tab, mr - 1, nr) - q0;
}

// etat[c][x][d] = {lg(eta+1) - lg(eta), lg(eta+1) - lg(eta+2)} of eta = eta[c][x][d]; thread = (chain, block, degree)
__global__ __launch_bounds__(256) void edge_eta_terms_kernel(EdgeProbParams p) {
    const size_t per = (size_t)(p.ka + p.kb) * (p.maxdeg + 1);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_range * per) return;
    if (p.rung && p.rung[p.c0 + i / per] != 0u) return;  // (not counted: never read)
    const long long e = p.eta[(size_t)p.c0 * per + i];
    const double l1 = lgamma_fast(p.tab, e + 1);
    p.etat[2 * i] = l1 - lgamma_fast(p.tab, e);
    p.etat[2 * i + 1] = l1 - lgamma_fast(p.tab, e + 2);
}

template <class LabelT, bool IN_LDS>
__global__ __launch_bounds__(256) void edge_probs_kernel(EdgeProbParams p) {
    extern __shared__ __align__(16) double lds[];  // IN_LDS: 2 x {block terms [K][4], m quadrant [ka][kb] (+ 1 when odd)}
    const uint32_t K = p.ka + p.kb, quad = p.ka * p.kb, D = p.maxdeg + 1;
    const uint32_t buf_doubles = K * 4 + (quad + 1) / 2;

    // lane t holds pairs tile * kEdgeProbsTile + j * 256 + t; past the end: nothing is computed or stored
    uint32_t pu[kPerLane], pv[kPerLane], du[kPerLane], dv[kPerLane], rem[kPerLane];
    double tdeg[kPerLane], tmult[kPerLane], acc_s[kPerLane], acc_w[kPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; ++j) {
        const uint32_t i = blockIdx.x * kEdgeProbsTile + j * kLanes + threadIdx.x;
        const bool in = i < p.n_pairs;
        pu[j] = in ? p.u[i] : 0u, pv[j] = in ? p.v[i] : 0u;
        du[j] = in ? p.du[i] : 0u, dv[j] = in ? p.dv[i] : 0u;
        rem[j] = in && p.kind[i] == BISBM_EDGE_REMOVE ? 1u : 0u;
        tdeg[j] = in ? p.tdeg[i] : 0., tmult[j] = in ? p.tmult[i] : 0.;
        acc_s[j] = in ? p.dS_sum[i] : 0., acc_w[j] = in ? p.w_sum[i] : 0.;
    }

    const double gain0 = lgamma_fast(p.tab, 1) - lgamma_fast(p.tab, 2);  // the second form of an eta entry outside 0 .. maxdeg (eta = 0)
    uint32_t buf = 0;
    for (uint32_t cb = 0; cb < p.n_range; ++cb) {
        const uint32_t c = p.c0 + cb;
        double* last = p.last ? p.last + (size_t)(p.row ? p.row[c] : c) * p.n_pairs : nullptr;
        if (p.rung && p.rung[c] != 0u) {  // (the same for every lane) not counted
            if (last)
                for (uint32_t j = 0; j < kPerLane; ++j) {
                    const uint32_t i = blockIdx.x * kEdgeProbsTile + j * kLanes + threadIdx.x;
                    if (i < p.n_pairs) last[i] = NAN;
                }
            continue;
        }
        const int32_t* m_t = p.m + (size_t)c * quad;
        const double* blk_t = p.blk + (size_t)cb * K * 4;
        if constexpr (IN_LDS) {
            // the buffer the chain before last used: every wave has passed the barrier of the last chain since it read it
            double* t = lds + (size_t)buf * buf_doubles;
            int32_t* m_l = (int32_t*)(t + (size_t)K * 4);
            for (uint32_t i = threadIdx.x; i < K * 4; i += kLanes) t[i] = blk_t[i];
            for (uint32_t i = threadIdx.x; i < quad; i += kLanes) m_l[i] = m_t[i];
            __syncthreads();
            m_t = m_l, blk_t = t;
            buf ^= 1u;
        }
        const LabelT* lab = (const LabelT*)p.labels + (size_t)c * p.label_stride;
        const double* et_c = p.etat + (size_t)cb * K * D * 2;
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j) {
            const uint32_t i = blockIdx.x * kEdgeProbsTile + j * kLanes + threadIdx.x;
            if (i >= p.n_pairs) continue;
            const uint32_t r = lab[pu[j]], s = lab[pv[j]];
            const long long mrs = m_t[r * p.kb + (s - p.ka)];
            // eta_x[d] is 0 outside 0 .. maxdeg (d - 1 of d = 0 wraps past it: a REMOVE pair has d >= 1 anyway)
            const uint32_t du2 = rem[j] ? du[j] - 1u : du[j] + 1u, dv2 = rem[j] ? dv[j] - 1u : dv[j] + 1u;
            const double* et_r = et_c + (size_t)r * D * 2;
            const double* et_s = et_c + (size_t)s * D * 2;
            const double t_m = lgamma_fast(p.tab, mrs + 1) - lgamma_fast(p.tab, rem[j] ? mrs : mrs + 2);
            const double* br = blk_t + (size_t)r * 4 + 2 * rem[j];
            const double* bs = blk_t + (size_t)s * 4 + 2 * rem[j];
            const double t_mr = br[0] + bs[0];
            const double t_eta = (et_r[2 * du[j]] + (du2 < D ? et_r[2 * du2 + 1] : gain0)) + (et_s[2 * dv[j]] + (dv2 < D ? et_s[2 * dv2 + 1] : gain0));
            const double t_q = br[1] + bs[1];
            const double dS = (((((tdeg[j] + t_m) + t_mr) + t_eta) + t_q) + tmult[j]) + p.tE[rem[j]];
            acc_s[j] += dS;
            acc_w[j] += (dS > 700.0) ? 0.0 : exp(-dS);
            if (last) last[i] = dS;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; ++j) {
        const uint32_t i = blockIdx.x * kEdgeProbsTile + j * kLanes + threadIdx.x;
        if (i < p.n_pairs) p.dS_sum[i] = acc_s[j], p.w_sum[i] = acc_w[j];
    }
}

// the block terms and the eta terms of the range of `p` (of p: the shape, the range, m_r, n_r, eta, rung, tab, blk, etat)
hipError_t launch_terms(const EdgeProbParams& p, hipStream_t stream) {
    const uint32_t K = p.ka + p.kb;
    hipLaunchKernelGGL(edge_block_terms_kernel, dim3((p.n_range * K + 255) / 256), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t cells = (size_t)p.n_range * K * (p.maxdeg + 1);
    hipLaunchKernelGGL(edge_eta_terms_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_edge_probs(const EdgeProbParams& p, bool wide, hipStream_t stream) {
    const uint32_t K = p.ka + p.kb;
    hipError_t e = launch_terms(p, stream);
    if (e != hipSuccess) return e;
    const dim3 grid((p.n_pairs + kEdgeProbsTile - 1) / kEdgeProbsTile), block(kLanes);
    if (wide) {
        hipLaunchKernelGGL((edge_probs_kernel<uint16_t, false>), grid, block, 0, stream, p);
        return hipGetLastError();
    }
    // byte labels: at most 256 blocks, so two copies of a chain's block terms (8 KiB) and quadrant (64 KiB) are at most 144 KiB of
    // the CU's 160 KiB
    const size_t lds = sizeof(double) * 2 * (4 * (size_t)K + ((size_t)p.ka * p.kb + 1) / 2);
    e = hipFuncSetAttribute((const void*)edge_probs_kernel<uint8_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((edge_probs_kernel<uint8_t, true>), grid, block, lds, stream, p);
    return hipGetLastError();
}

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream
int add_sample(bisbm_engine* h, bisbm_engine* e) {
    EdgeProbState& s = h->edges;
    if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_edge_probs_accumulate");
    const uint32_t K = e->ka + e->kb;
    const size_t eta_cells = (size_t)K * (e->maxdeg + 1);  // per chain
    const uint32_t per = edge_range_chains(e);
    RESERVE(h, s.d_blk, (size_t)per * K * 4);
    RESERVE(h, s.d_etat, (size_t)per * eta_cells * 2);
    const HostTables& tab = *h->tab;
    const uint64_t E = h->num_edges, cells = (uint64_t)e->ka * e->kb;
    EdgeProbParams p{};
    p.n_pairs = (uint32_t)s.n;
    p.ka = e->ka, p.kb = e->kb, p.maxdeg = e->maxdeg;
    p.u = s.d_u.get(), p.v = s.d_v.get(), p.du = s.d_du.get(), p.dv = s.d_dv.get();
    p.kind = s.d_kind.get();
    p.tdeg = s.d_tdeg.get(), p.tmult = s.d_tmult.get();
    p.labels = e->d_labels;
    p.label_stride = e->label_stride;
    p.m = e->d_m, p.m_r = e->d_m_r, p.n_r = e->d_n_r, p.eta = e->d_eta;
    p.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    p.tab = Tables{e->d_lgamma, tab.lg.size(), e->d_q, e->q_stride, e->d_logtab};
    // the edge-count prior of this shape (entropy_terms: t[2] = lbinom(ka kb + E - 1, E)); REMOVE is only listed where E >= 1
    const double tE0 = h_lbinom_fast(tab, cells + E - 1, E);
    p.tE[0] = h_lbinom_fast(tab, cells + E, E + 1) - tE0;
    p.tE[1] = E ? h_lbinom_fast(tab, cells + E - 2, E - 1) - tE0 : 0.;
    p.blk = s.d_blk.get(), p.etat = s.d_etat.get(), p.dS_sum = s.d_dS_sum.get(), p.w_sum = s.d_w_sum.get();
    if (s.what & BISBM_EDGE_KEEP_LAST) {  // every chain's dS to its row of the device entry
        p.last = s.d_last.get();
        if (e != h) {
            RESERVE(h, s.d_row, e->n_chains);
            HIPCHK(h, hipMemcpyAsync(s.d_row.get(), e->ridx.data(), sizeof(uint32_t) * e->n_chains, hipMemcpyHostToDevice, h->stream));
            p.row = s.d_row.get();
        }
    }
    for (uint32_t c0 = 0; c0 < e->n_chains; c0 += per) {  // (the ranges in ascending order, one after the other on the stream)
        p.c0 = c0, p.n_range = std::min(per, e->n_chains - c0);
        HIPCHK(h, launch_edge_probs(p, e->wide, h->stream));
    }
    if (e != h) HIPCHK(h, hipStreamSynchronize(h->stream));  // (the next group sizes and fills d_blk, d_etat and d_row anew)
    s.terms += e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    return BISBM_OK;
}

}  // namespace

namespace bisbm {

// chains per launch (BISBM_EDGE_RANGE_CHAINS=<n> in the environment, read at every call: n instead, for the tests)
uint32_t edge_range_chains(const bisbm_engine* e) {
    size_t range = kEtaTermBytes / (2 * sizeof(double) * (size_t)(e->ka + e->kb) * (e->maxdeg + 1));
    if (const char* env = std::getenv("BISBM_EDGE_RANGE_CHAINS")) range = std::strtoull(env, nullptr, 10);
    return (uint32_t)std::min<size_t>(std::max<size_t>(range, 1), e->n_chains);
}

hipError_t launch_edge_terms(const EdgeTermParams& t, hipStream_t stream) {
    EdgeProbParams p{};
    p.ka = t.ka, p.kb = t.kb, p.maxdeg = t.maxdeg, p.c0 = t.c0, p.n_range = t.n_range;
    p.m_r = t.m_r, p.n_r = t.n_r, p.eta = t.eta, p.rung = t.rung, p.tab = t.tab;
    p.blk = t.blk, p.etat = t.etat;
    return launch_terms(p, stream);
}

}  // namespace bisbm

extern "C" {

int bisbm_edge_probs_set(bisbm_handle h, uint64_t n_pairs, const uint32_t* u, const uint32_t* v, const uint8_t* kind, uint32_t what) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (n_pairs && (!u || !v)) return fail(h, BISBM_ERR_INVALID_ARG, "u or v is NULL");
    if (what & ~BISBM_EDGE_KEEP_LAST) return fail(h, BISBM_ERR_INVALID_ARG, "unknown bits 0x%x in what", what & ~BISBM_EDGE_KEEP_LAST);
    if (n_pairs >= 0xFFFFFFFFull) return fail(h, BISBM_ERR_UNSUPPORTED, "more than 2^32-2 pairs");
    for (uint64_t i = 0; i < n_pairs; ++i) {  // (before anything changes: a refused call leaves the earlier pairs in place)
        if (u[i] >= h->na || v[i] < h->na || v[i] >= h->n)
            return fail(h, BISBM_ERR_INVALID_ARG, "pair %llu = (%u, %u): u must be a type-a node [0, %llu), v a type-b node [%llu, %llu)",
                        (unsigned long long)i, u[i], v[i], (unsigned long long)h->na, (unsigned long long)h->na, (unsigned long long)h->n);
        if (kind && kind[i] != BISBM_EDGE_ADD && kind[i] != BISBM_EDGE_REMOVE)
            return fail(h, BISBM_ERR_INVALID_ARG, "pair %llu = (%u, %u): unknown kind %u", (unsigned long long)i, u[i], v[i], kind[i]);
    }
    if (!h->devs.empty()) {  // (every device entry checks the same graph: all refuse, or none)
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_edge_probs_set(d, n_pairs, u, v, kind, what); });
        if (rc == BISBM_OK) h->edges.n = n_pairs;
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_pairs == 0) {
        h->edges = EdgeProbState();  // (the old pairs, their sums and buffers go)
        return BISBM_OK;
    }
    EdgeProbState s;  // built aside: it replaces the old pairs once every REMOVE has found its edge
    const size_t P = (size_t)n_pairs;
    // sorted by (u, v), equal pairs in the caller's order
    std::vector<std::pair<uint64_t, uint32_t>> keyed(P);
    for (size_t i = 0; i < P; ++i) keyed[i] = {(uint64_t)u[i] << 32 | v[i], (uint32_t)i};
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> su(P), sv(P);
    std::vector<uint8_t> sk(P);
    s.order.resize(P), s.pos.resize(P), s.mult.resize(P);
    for (size_t i = 0; i < P; ++i) {
        su[i] = (uint32_t)(keyed[i].first >> 32), sv[i] = (uint32_t)keyed[i].first, s.order[i] = keyed[i].second;
        sk[i] = kind ? kind[s.order[i]] : (uint8_t)BISBM_EDGE_ADD;
        s.pos[s.order[i]] = (uint32_t)i;
    }
    DeviceBuf<uint32_t> d_mult;
    hipError_t e = s.d_u.reserve(P);
    if (e == hipSuccess) e = s.d_v.reserve(P);
    if (e == hipSuccess) e = s.d_du.reserve(P);
    if (e == hipSuccess) e = s.d_dv.reserve(P);
    if (e == hipSuccess) e = d_mult.reserve(P);
    if (e == hipSuccess) e = s.d_kind.reserve(P);
    if (e == hipSuccess) e = s.d_tdeg.reserve(P);
    if (e == hipSuccess) e = s.d_tmult.reserve(P);
    if (e == hipSuccess) e = s.d_dS_sum.reserve(P);
    if (e == hipSuccess) e = s.d_w_sum.reserve(P);
    if (e == hipSuccess && (what & BISBM_EDGE_KEEP_LAST)) e = s.d_last.reserve((size_t)h->n_chains * P);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_u.get(), su.data(), sizeof(uint32_t) * P, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_v.get(), sv.data(), sizeof(uint32_t) * P, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_kind.get(), sk.data(), P, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_dS_sum.get(), 0, sizeof(double) * P, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_w_sum.get(), 0, sizeof(double) * P, h->stream);
    EdgePairParams pp{(uint32_t)P, h->d_rowptr, h->d_col, s.d_u.get(), s.d_v.get(), s.d_kind.get(), h->d_lgamma, h->tab->lg.size(),
                      s.d_du.get(), s.d_dv.get(), d_mult.get(), s.d_tdeg.get(), s.d_tmult.get()};
    if (e == hipSuccess) {
        hipLaunchKernelGGL(edge_pairs_kernel, dim3(((uint32_t)P + 255) / 256), dim3(256), 0, h->stream, pp);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s.mult.data(), d_mult.get(), sizeof(uint32_t) * P, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, BISBM_ERR_HIP, "bisbm_edge_probs_set: %s", hipGetErrorString(e));
    if (kind) {
        size_t bad = P;  // the first REMOVE, in the caller's order, of an edge that is not there
        for (size_t i = 0; i < P; ++i)
            if (sk[i] == BISBM_EDGE_REMOVE && s.mult[i] == 0) bad = std::min<size_t>(bad, s.order[i]);
        if (bad < P)
            return fail(h, BISBM_ERR_INVALID_ARG, "pair %llu = (%u, %u): REMOVE of an edge the graph does not hold", (unsigned long long)bad, u[bad], v[bad]);
    }
    s.n = n_pairs, s.what = what;
    h->edges = std::move(s);
    return BISBM_OK;
}

int bisbm_edge_probs_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->edges.n) return fail(h, BISBM_ERR_STATE, "no pairs listed: call bisbm_edge_probs_set first");
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_edge_probs_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->edges.have_last = (h->edges.what & BISBM_EDGE_KEEP_LAST) != 0;
    return BISBM_OK;
}

int bisbm_edge_probs_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_edge_probs_reset(d); });
    h->edges.terms = 0;
    if (!h->edges.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->edges.d_dS_sum.get(), 0, sizeof(double) * h->edges.n, h->stream));
    HIPCHK(h, hipMemsetAsync(h->edges.d_w_sum.get(), 0, sizeof(double) * h->edges.n, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_edge_probs_get(bisbm_handle h, double* dS_sum, double* w_sum, uint32_t* mult_out, uint64_t* terms) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->edges.n) return fail(h, BISBM_ERR_STATE, "no pairs listed: call bisbm_edge_probs_set first");
    const size_t P = (size_t)h->edges.n;
    if (!h->devs.empty()) {  // the per-device sums are added on the host in device order
        std::vector<double> part_s(dS_sum ? P : 0), part_w(w_sum ? P : 0);
        uint64_t total = 0;
        if (dS_sum) std::fill(dS_sum, dS_sum + P, 0.);
        if (w_sum) std::fill(w_sum, w_sum + P, 0.);
        for (size_t k = 0; k < h->devs.size(); ++k) {
            bisbm_engine* d = h->devs[k];
            uint64_t t = 0;
            if (int rc = bisbm_edge_probs_get(d, dS_sum ? part_s.data() : nullptr, w_sum ? part_w.data() : nullptr, k ? nullptr : mult_out, &t)) {
                h->err = d->err;
                return rc;
            }
            total += t;
            for (size_t i = 0; dS_sum && i < P; ++i) dS_sum[i] += part_s[i];
            for (size_t i = 0; w_sum && i < P; ++i) w_sum[i] += part_w[i];
        }
        if (terms) *terms = total;
        return BISBM_OK;
    }
    const EdgeProbState& s = h->edges;
    if (terms) *terms = s.terms;
    if (mult_out)
        for (size_t i = 0; i < P; ++i) mult_out[s.order[i]] = s.mult[i];
    if (!dS_sum && !w_sum) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<double> sorted(P);
    for (int k = 0; k < 2; ++k) {
        double* out = k ? w_sum : dS_sum;
        if (!out) continue;
        HIPCHK(h, hipMemcpy(sorted.data(), (k ? s.d_w_sum : s.d_dS_sum).get(), sizeof(double) * P, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < P; ++i) out[s.order[i]] = sorted[i];
    }
    return BISBM_OK;
}

int bisbm_edge_probs_get_last(bisbm_handle h, uint64_t pair_index, double* dS_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->edges.n) return fail(h, BISBM_ERR_STATE, "no pairs listed: call bisbm_edge_probs_set first");
    if (!dS_out) return fail(h, BISBM_ERR_INVALID_ARG, "dS_out is NULL");
    if (pair_index >= h->edges.n) return fail(h, BISBM_ERR_INVALID_ARG, "pair_index %llu >= %llu pairs", (unsigned long long)pair_index, (unsigned long long)h->edges.n);
    if (!h->devs.empty()) {
        for (size_t k = 0; k < h->devs.size(); ++k)
            if (int rc = bisbm_edge_probs_get_last(h->devs[k], pair_index, dS_out + h->dev_first[k])) {
                h->err = h->devs[k]->err;
                return rc;
            }
        return BISBM_OK;
    }
    const EdgeProbState& s = h->edges;
    if (!s.have_last)
        return fail(h, BISBM_ERR_STATE, "no sample on record: call bisbm_edge_probs_set with BISBM_EDGE_KEEP_LAST, then bisbm_edge_probs_accumulate");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t c = 0; c < h->n_chains; ++c)  // (one value per chain: a column of d_last)
        HIPCHK(h, hipMemcpy(dS_out + c, s.d_last.get() + (size_t)c * s.n + s.pos[(size_t)pair_index], sizeof(double), hipMemcpyDeviceToHost));
    return BISBM_OK;
}

}  // extern "C"
