// bisbm_conditionals.hip -- node conditionals: for an existing node v and one chain, the change of the description length
// dS(v: r -> s) for EVERY block s of v's type at once, the full conditional P(b_v = s | all other labels) ~ exp(-beta dS_s) that
// follows from it, its label-free terms (stay, entropy, margin) pooled over the chains, the rows themselves pushed through the
// alignment permutations into a soft marginal histogram, and the last sample's rows per chain (no reference counterpart;
// include/bisbm.h, "Node conditionals", states every f64 operation and its order).  Chain state is only read.
//
// Rows kernel: one workgroup per (chain, query), of 64 lanes where neither type has more than 64 blocks and of 256 otherwise.  Shared by all targets of the node: the walk over its CSR row, the
// k_v histogram (integer LDS atomics, as mh_step builds it; rows of any length), the list of the non-zero (t, k_t) compacted in
// ascending t (ballots, so the list order does not depend on timing), the two lgamma values of the r side per t, and the r-side
// scalar and log_q terms.  Then lane <-> target s (a type has at most 255 blocks while the labels are bytes): per non-zero t
// two table gathers and one f64 add, in list order inside the lane, then the three scalar pairs.  The chain's quadrant of m is
// read through L1 / L2, not staged: a workgroup needs row r and |{t : k_t != 0}| columns of it, the up to 64 KiB are shared by
// the queries of the chain, whose workgroups are neighbours in the grid, and 64 KiB of LDS per workgroup would leave two
// workgroups per CU (the reasoning of bisbm_foldin.hip's table kernel).  min, Z and the entropy are taken by one lane in ascending
// s: their order is part of the definition.
//
// Pool kernel: one lane per query walks the chains of the launch in ascending order and adds the counted chains' terms, one f64
// add each.  Soft kernel: one workgroup per query, lane <-> block s; a chain's permutation is a bijection, so the lanes of one
// chain write different columns and every column sees the chains in ascending order.
#include "bisbm_engine.hpp"
#include "bisbm_wave_chain.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256;
constexpr size_t kScratchBudget = 256ull << 20;  // bytes of rows and terms of one chunk of chains (at least one chain)
constexpr uint32_t kMaxChunk = 65535;            // chains of one launch: the grid's y

__device__ __forceinline__ double nan_row() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ double logq_of(const Tables& tab, int n, int k) {
    return log_q<true>(tab, n, k, log_n_of(tab, n));
}

// kLanes: 64 where neither type has more than 64 blocks (one wave: four times as many workgroups fit a CU, and the barriers cost
// nothing), else 256
// HELD: the launch has a clamp, block constraints or block fields and bisbm_held_conditionals_set is on (include/bisbm.h, "Held
// conditionals"): the row is the heat-bath kernel's -- the field added in the target's lane, the minimum, the margin and the weights
// restricted to A_v, a clamped node or one with a single allowed block a point mass.  The instances without it hold none of its code.
template <uint32_t kLanes, bool HELD>
__global__ __launch_bounds__(kLanes) void cond_rows_kernel(CondRowsParams p) {
    __shared__ int s_k[kLanes];          // k_v histogram over the blocks of the other type
    __shared__ uint32_t s_t[kLanes];     // the non-zero t, ascending
    __shared__ int s_kt[kLanes];         // their k_t
    __shared__ double s_L1[kLanes], s_L3[kLanes];  // lg(m_rt + 1), lg(m_rt - k_t + 1) per list entry
    __shared__ double s_x[kLanes];       // dS, then w, then P per target
    __shared__ uint32_t s_wcnt[kLanes / 64];
    __shared__ double s_min, s_margin, s_Z;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t qi = blockIdx.x, c = p.chain0 + blockIdx.y, bc = c - p.buf_chain0;
    const uint32_t v = p.q[qi], nbb = p.nbb[qi];
    const bool tb = v >= p.na;
    const uint32_t K = p.ka + p.kb, D = p.maxdeg + 1;
    const uint32_t k_own = tb ? p.kb : p.ka, k_oth = tb ? p.ka : p.kb, own0 = tb ? p.ka : 0u, oth0 = tb ? 0u : p.ka;
    const size_t row_at = (size_t)bc * p.row_total + (size_t)(qi - nbb) * p.ka + (size_t)nbb * p.kb;
    double* dS_row = p.dS + row_at;
    double* P_row = p.P + row_at;
    double* terms = p.terms + ((size_t)blockIdx.y * p.n_q + qi) * 4;
    if (p.rung && p.rung[c] != 0u) {  // (the same for every lane) not counted: NaN rows
        if (tid < k_own) dS_row[tid] = nan_row(), P_row[tid] = nan_row();
        if (tid < 4) terms[tid] = nan_row();
        return;
    }
    const Tables tab{p.lgamma_tab, p.lgamma_size, p.q_tab, p.q_stride, p.log_tab};
    const uint8_t* lab = p.labels + (size_t)c * p.label_stride;
    const int32_t* m_g = p.m + (size_t)c * p.ka * p.kb;
    const int32_t* mr_g = p.m_r + (size_t)c * K;
    const int32_t* nr_g = p.n_r + (size_t)c * K;
    const uint32_t* eta_g = p.eta + (size_t)c * K * D;
    const uint32_t beg = p.rowptr[v], deg = p.rowptr[v + 1] - beg;
    const uint32_t r_loc = min((uint32_t)lab[v] - own0, k_own - 1u), r = own0 + r_loc;  // (a valid label: the min never binds)
    // held rows: the node's mask byte, class and field row (v is the workgroup's: one read each), and its own entry of A_v
    bool held_shut = false, ok = true;  // clamped or |A_v| = 1; block tid is in A_v (the node's own block always is)
    const double* f_row = nullptr;
    uint8_t* s_ok = nullptr;
    if constexpr (HELD) {
        __shared__ uint8_t s_ok_[kLanes];
        s_ok = s_ok_;
        held_shut = p.clamp && p.clamp[v] != 0;
        if (p.cn_bits) {
            const uint32_t cls = p.cn_class[v];
            held_shut = held_shut || cn_count(p.cn_bits, cls, own0, k_own) <= 1u;
            ok = tid == r_loc || (tid < k_own && cn_allows(p.cn_bits, cls, own0 + tid));
        }
        s_ok[tid] = ok ? 1 : 0;  // (read behind the barriers below)
        if (p.fl_field) f_row = p.fl_field + (size_t)p.fl_class[v] * K;
    }

    // 1. k_v: the histogram of the neighbours' labels
    s_k[tid] = 0;
    __syncthreads();
    for (uint32_t j = tid; j < deg; j += kLanes) {
        const uint32_t t = (uint32_t)lab[p.col[beg + j]] - oth0;
        if (t < k_oth) atomicAdd(&s_k[t], 1);
    }
    __syncthreads();
    // 2. the non-zero (t, k_t) in ascending t, with the r side's two table values
    const int kt = tid < k_oth ? s_k[tid] : 0;
    const unsigned long long bal = __ballot(kt != 0);
    if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t pos = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), nnz = 0;
    for (uint32_t w = 0; w < kLanes / 64; ++w) {
        if (w < wave) pos += s_wcnt[w];
        nnz += s_wcnt[w];
    }
    if (kt != 0) {
        const int32_t m_rt = tb ? m_g[tid * p.kb + r_loc] : m_g[r_loc * p.kb + tid];
        s_t[pos] = tid, s_kt[pos] = kt;
        s_L1[pos] = lgamma_fast(tab, (long long)m_rt + 1);
        s_L3[pos] = lgamma_fast(tab, (long long)m_rt - kt + 1);
    }
    __syncthreads();
    // 3. dS of target s = tid
    const int ideg = (int)deg;
    const int m0r = mr_g[r], n0r = nr_g[r];
    double dS = 0.;
    if (tid < k_own && tid != r_loc) {
        const uint32_t s = own0 + tid;
        double acc = 0.;
        // four list entries at a time: their reads of m and the eight table gathers are in flight together; the adds keep the
        // list order
        uint32_t i = 0;
        for (; i + 4 <= nnz; i += 4) {
            int32_t m_st[4];
            double a[4], b[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t t = s_t[i + j];
                m_st[j] = tb ? m_g[t * p.kb + tid] : m_g[tid * p.kb + t];
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                a[j] = lgamma_fast(tab, (long long)m_st[j] + 1);
                b[j] = lgamma_fast(tab, (long long)m_st[j] + s_kt[i + j] + 1);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) acc = acc + ((s_L1[i + j] + a[j]) - (s_L3[i + j] + b[j]));
        }
        for (; i < nnz; ++i) {
            const uint32_t t = s_t[i];
            const int k = s_kt[i];
            const int32_t m_st = tb ? m_g[t * p.kb + tid] : m_g[tid * p.kb + t];
            acc = acc + ((s_L1[i] + lgamma_fast(tab, (long long)m_st + 1)) - (s_L3[i] + lgamma_fast(tab, (long long)m_st + k + 1)));
        }
        const int m0s = mr_g[s], n0s = nr_g[s];
        const long long eta_r = eta_g[(size_t)r * D + deg], eta_s = eta_g[(size_t)s * D + deg];
        const double tail1 = (lgamma_fast(tab, (long long)m0r - ideg + 1) - lgamma_fast(tab, (long long)m0r + 1)) +
                             (lgamma_fast(tab, (long long)m0s + ideg + 1) - lgamma_fast(tab, (long long)m0s + 1));
        const double tail2 = (lgamma_fast(tab, eta_r + 1) - lgamma_fast(tab, eta_r)) + (lgamma_fast(tab, eta_s + 1) - lgamma_fast(tab, eta_s + 2));
        const double tail3 = (logq_of(tab, m0r - ideg, n0r - 1) - logq_of(tab, m0r, n0r)) + (logq_of(tab, m0s + ideg, n0s + 1) - logq_of(tab, m0s, n0s));
        dS = ((acc + tail1) + tail2) + tail3;
        if constexpr (HELD)
            if (f_row) dS = dS + (f_row[s] - f_row[r]);  // (the difference first, then one add: "Block fields" 2.)
    }
    if (tid < k_own) dS_row[tid] = dS;
    s_x[tid] = dS;
    __syncthreads();
    // 4. the conditional: min, weights, Z in ascending s, P; then the chain's label-free terms
    const bool free_node = k_own > 1u && n0r > 1 && !(HELD && held_shut);
    if (tid == 0) {
        double mn = 0., mg = 0.;  // (the 0 at r)
        bool first = true;
#pragma unroll 8
        for (uint32_t s = 0; s < k_own; ++s) {
            if (s == r_loc) continue;
            if constexpr (HELD)
                if (!s_ok[s]) continue;  // (the minimum and the margin are over A_v)
            const double x = s_x[s];
            mn = x < mn ? x : mn;
            mg = (first || x < mg) ? x : mg;
            first = false;
        }
        s_min = mn, s_margin = mg;
    }
    __syncthreads();
    double w = tid == r_loc ? 1. : 0.;
    if (free_node && tid < k_own) {
        const double x = p.beta * (dS - s_min);
        w = x > 700. || (HELD && !ok) ? 0. : exp(-x);  // (exactly 0.0 outside A_v)
    }
    __syncthreads();
    s_x[tid] = w;
    __syncthreads();
    if (tid == 0) {
        double Z = s_x[0];
#pragma unroll 8
        for (uint32_t s = 1; s < k_own; ++s) Z = Z + s_x[s];
        s_Z = Z;
    }
    __syncthreads();
    const double Pv = free_node ? w / s_Z : w;
    if (tid < k_own) P_row[tid] = Pv;
    __syncthreads();
    s_x[tid] = Pv;
    __syncthreads();
    if (tid == 0) {
        double acc = 0.;
        for (uint32_t s = 0; s < k_own; ++s) {
            const double x = s_x[s];
            if (x != 0.) acc = acc + x * log(x);
        }
        terms[0] = s_x[r_loc];
        terms[1] = 0. - acc;
        terms[2] = free_node ? s_margin : 0.;
        terms[3] = free_node ? 1. : 0.;
    }
}

// the terms of the launch's chains onto the kept sums: lane = query, chains in ascending order
__global__ __launch_bounds__(256) void cond_pool_kernel(const double* terms, uint32_t n_q, uint32_t n_chains, double* stat, unsigned long long* free_cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    double stay = stat[q], ent = stat[(size_t)n_q + q], mar = stat[2 * (size_t)n_q + q];
    unsigned long long fr = free_cnt[q];
    for (uint32_t c = 0; c < n_chains; ++c) {
        const double* t = terms + ((size_t)c * n_q + q) * 4;
        const double t0 = t[0];
        if (t0 != t0) continue;  // (a chain that was not counted)
        stay = stay + t0;
        ent = ent + t[1];
        if (t[3] != 0.) mar = mar + t[2], fr += 1;
    }
    stat[q] = stay, stat[(size_t)n_q + q] = ent, stat[2 * (size_t)n_q + q] = mar;
    free_cnt[q] = fr;
}

// prob[q][perm_c(s) - type base] += P_c(s): workgroup = query, lane = s, chains in ascending order
__global__ __launch_bounds__(256) void cond_soft_kernel(CondSoftParams p) {
    const uint32_t qi = blockIdx.x, s = threadIdx.x;
    const uint32_t v = p.q[qi], nbb = p.nbb[qi];
    const bool tb = v >= p.na;
    const uint32_t K = p.ka + p.kb, k_own = tb ? p.kb : p.ka, own0 = tb ? p.ka : 0u;
    if (s >= k_own) return;
    const size_t row_at = (size_t)(qi - nbb) * p.ka + (size_t)nbb * p.kb + s;
    double* out = p.prob + (size_t)qi * p.kmax;
    for (uint32_t cl = 0; cl < p.n_chains; ++cl) {
        const uint32_t c = p.chain0 + cl;
        const double x = p.P[(size_t)(c - p.buf_chain0) * p.row_total + row_at];
        if (x != x) continue;  // (a chain that was not counted)
        const uint32_t j = (uint32_t)p.perm[(size_t)c * K + own0 + s] - own0;
        if (j < p.kmax) out[j] = out[j] + x;
    }
}

// the device's logarithm for a host that restates the entropy term (bisbm_debug_log)
__global__ void log_probe_kernel(const double* x, size_t count, double* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = log(x[i]);
}

}  // namespace

namespace bisbm {

hipError_t launch_cond_rows(const CondRowsParams& p, hipStream_t stream) {
    if (p.n_q == 0 || p.n_chains == 0) return hipSuccess;
    const bool held = p.clamp || p.cn_bits || p.fl_field;  // (the switch on with nothing held: the plain instances)
    if (std::max(p.ka, p.kb) <= 64u) {
        if (held)
            hipLaunchKernelGGL((cond_rows_kernel<64, true>), dim3(p.n_q, p.n_chains), dim3(64), 0, stream, p);
        else
            hipLaunchKernelGGL((cond_rows_kernel<64, false>), dim3(p.n_q, p.n_chains), dim3(64), 0, stream, p);
    } else {
        if (held)
            hipLaunchKernelGGL((cond_rows_kernel<256, true>), dim3(p.n_q, p.n_chains), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((cond_rows_kernel<256, false>), dim3(p.n_q, p.n_chains), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_cond_pool(const double* terms, uint32_t n_q, uint32_t n_chains, double* stat, unsigned long long* free_cnt, hipStream_t stream) {
    if (n_q == 0 || n_chains == 0) return hipSuccess;
    hipLaunchKernelGGL(cond_pool_kernel, dim3((n_q + 255) / 256), dim3(256), 0, stream, terms, n_q, n_chains, stat, free_cnt);
    return hipGetLastError();
}

hipError_t launch_cond_soft(const CondSoftParams& p, hipStream_t stream) {
    if (p.n_q == 0 || p.n_chains == 0) return hipSuccess;
    hipLaunchKernelGGL(cond_soft_kernel, dim3(p.n_q), dim3(kLanes), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bisbm

namespace {

const char* kNoQueries = "no queries: call bisbm_conditionals_set first";

size_t row_total(const ConditionalState& s, uint32_t ka, uint32_t kb) { return (size_t)(s.n - s.n_b) * ka + (size_t)s.n_b * kb; }

// the permutations of every chain of `e` to the reference, into s.scratch.d_perm[chain][ka + kb] (list position = chain)
int align_chains(bisbm_engine* h, bisbm_engine* e) {
    ConditionalState& s = h->cond;
    AlignScratch& a = s.scratch;
    const uint32_t ka = e->ka, kb = e->kb, C = e->n_chains;
    const size_t T = (size_t)ka * ka + (size_t)kb * kb;
    if (a.ref_uploaded != s.ref_serial) {
        RESERVE(h, a.d_ref, e->label_stride);
        std::vector<uint8_t> ref(e->label_stride, 0);
        for (uint64_t v = 0; v < e->n; ++v) ref[v] = (uint8_t)s.ref.labels[v];
        HIPCHK(h, hipMemcpyAsync(a.d_ref.get(), ref.data(), ref.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        a.ref_uploaded = s.ref_serial;
    }
    if (a.list.size() != C) {
        a.list.resize(C);
        for (uint32_t c = 0; c < C; ++c) a.list[c] = c;
        RESERVE(h, a.d_list, C);
        RESERVE(h, a.d_mode, C);
        HIPCHK(h, hipMemcpyAsync(a.d_list.get(), a.list.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(a.d_mode.get(), 0, sizeof(uint32_t) * C, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    RESERVE(h, a.d_tab, (size_t)C * T);
    RESERVE(h, a.d_perm, (size_t)C * (ka + kb));
    RESERVE(h, a.d_tot, (size_t)C * 2);
    HIPCHK(h, hipMemsetAsync(a.d_tab.get(), 0, sizeof(uint32_t) * C * T, h->stream));
    OverlapParams op{};
    op.labels = e->d_labels, op.label_stride = e->label_stride;
    op.ref = a.d_ref.get(), op.list = a.d_list.get(), op.ref_row = a.d_mode.get();
    op.n = (uint32_t)e->n, op.na = (uint32_t)e->na, op.ka = ka, op.kb = kb;
    op.tab = a.d_tab.get();
    HIPCHK(h, launch_overlap(op, C, h->stream));
    HIPCHK(h, launch_align_assign(a.d_tab.get(), ka, kb, a.d_perm.get(), a.d_tot.get(), C, h->stream));
    return BISBM_OK;
}

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the sums of `h`, on h's stream; with
// last rows kept they go to segment `seg` of h's row buffers
int add_sample(bisbm_engine* h, bisbm_engine* e, const ConditionalState::Segment& seg) {
    ConditionalState& s = h->cond;
    const bool keep = (s.what & BISBM_COND_KEEP_LAST) != 0;
    const size_t rt = row_total(s, e->ka, e->kb);
    const size_t per_chain = sizeof(double) * 4 * (size_t)s.n + (keep ? 0 : 2 * sizeof(double) * rt);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(std::min(e->n_chains, kMaxChunk), std::max<uint64_t>(1, kScratchBudget / per_chain));
    RESERVE(h, s.d_terms, (size_t)chunk * s.n * 4);
    if (!keep) {
        RESERVE(h, s.d_dS, (size_t)chunk * rt);
        RESERVE(h, s.d_P, (size_t)chunk * rt);
    }
    if (s.ref.has)
        if (int rc = align_chains(h, e)) return rc;
    CondRowsParams p{};
    p.na = (uint32_t)h->na, p.ka = e->ka, p.kb = e->kb, p.maxdeg = e->maxdeg;
    p.n_q = s.n, p.beta = s.beta, p.row_total = rt;
    p.q = s.d_q.get(), p.nbb = s.d_nbb.get();
    p.rowptr = h->d_rowptr, p.col = h->d_col;
    p.labels = e->d_labels, p.label_stride = e->label_stride;
    p.m = e->d_m, p.m_r = e->d_m_r, p.n_r = e->d_n_r, p.eta = e->d_eta;
    p.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    p.lgamma_tab = e->d_lgamma, p.lgamma_size = e->tab->lg.size(), p.q_tab = e->d_q, p.q_stride = e->q_stride, p.log_tab = e->d_logtab;
    p.dS = s.d_dS.get() + (keep ? seg.base : 0), p.P = s.d_P.get() + (keep ? seg.base : 0);
    p.terms = s.d_terms.get();
    if (s.held) {  // (the pointers the heat-bath launch takes; holds are refused on grouped handles, so `e` is the handle itself)
        p.clamp = e->clamp.mask_or_null();
        p.cn_class = e->constraints.class_or_null(), p.cn_bits = e->constraints.bits_or_null();
        p.fl_class = e->fields.class_or_null(), p.fl_field = e->fields.field_or_null();
    }
    CondSoftParams sp{};
    sp.na = p.na, sp.ka = e->ka, sp.kb = e->kb, sp.kmax = std::max(e->ka, e->kb), sp.n_q = s.n, sp.row_total = rt;
    sp.q = p.q, sp.nbb = p.nbb, sp.P = p.P, sp.perm = s.scratch.d_perm.get(), sp.prob = s.d_prob.get();
    for (uint32_t c0 = 0; c0 < e->n_chains; c0 += chunk) {
        p.chain0 = sp.chain0 = c0;
        p.n_chains = sp.n_chains = std::min(chunk, e->n_chains - c0);
        p.buf_chain0 = sp.buf_chain0 = keep ? 0u : c0;
        HIPCHK(h, launch_cond_rows(p, h->stream));
        HIPCHK(h, launch_cond_pool(s.d_terms.get(), s.n, p.n_chains, s.d_stat.get(), s.d_free.get(), h->stream));
        if (s.ref.has) HIPCHK(h, launch_cond_soft(sp, h->stream));
    }
    const uint64_t counted = e->temper.L ? e->n_chains / e->temper.L : e->n_chains;  // (every ensemble has one chain on rung 0)
    s.terms += counted;
    if (s.ref.has) s.prob_terms += counted;
    return BISBM_OK;
}

int zero_prob(bisbm_engine* h) {
    ConditionalState& s = h->cond;
    s.prob_terms = 0;
    if (s.d_prob && s.prob_cells) HIPCHK(h, hipMemsetAsync(s.d_prob.get(), 0, sizeof(double) * s.prob_cells, h->stream));
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_conditionals_set(bisbm_handle h, uint32_t n_queries, const uint32_t* queries, double beta, uint32_t what) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    ConditionalState f;
    if (n_queries) {  // (before anything changes: a refused call leaves the earlier queries in place)
        if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
            return fail(h, BISBM_ERR_UNSUPPORTED, "node conditionals are defined in the Philox-mode arithmetic: this handle runs BISBM_RNG_MT19937_COMPAT");
        if (!(beta > 0.) || !std::isfinite(beta)) return fail(h, BISBM_ERR_INVALID_ARG, "beta = %g: a finite value above 0 is needed", beta);
        if (what & ~BISBM_COND_KEEP_LAST) return fail(h, BISBM_ERR_INVALID_ARG, "what = %u: the only bit is BISBM_COND_KEEP_LAST (1)", what);
        if (!queries && n_queries != h->n)
            return fail(h, BISBM_ERR_INVALID_ARG, "queries is NULL (every node) but n_queries = %u is not n = %llu", n_queries, (unsigned long long)h->n);
        if (queries)
            for (uint32_t i = 0; i < n_queries; ++i)
                if (queries[i] >= h->n) return fail(h, BISBM_ERR_INVALID_ARG, "query %u: node %u is out of range (n = %llu)", i, queries[i], (unsigned long long)h->n);
        f.n = n_queries, f.what = what, f.beta = beta;
        f.q.resize(n_queries);
        f.nbb.resize((size_t)n_queries + 1);
        for (uint32_t i = 0; i < n_queries; ++i) {
            f.q[i] = queries ? queries[i] : i;
            f.nbb[i] = f.n_b;
            f.n_b += f.q[i] >= h->na;
        }
        f.nbb[n_queries] = f.n_b;
    }
    if (!h->devs.empty()) {
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_conditionals_set(d, n_queries, queries, beta, what); });
        h->cond = ConditionalState();
        if (rc == BISBM_OK && n_queries) h->cond = std::move(f);
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->cond = ConditionalState();  // (the old queries, their sums, the reference and the buffers go)
    if (n_queries == 0) return BISBM_OK;
    hipError_t e = f.d_q.reserve(n_queries);
    if (e == hipSuccess) e = f.d_nbb.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = f.d_stat.reserve(3 * (size_t)n_queries);
    if (e == hipSuccess) e = f.d_free.reserve(n_queries);
    if (e != hipSuccess)
        return fail(h, BISBM_ERR_HIP, "bisbm_conditionals_set: %zu bytes of device memory for the sums of %u queries could not be allocated: %s",
                    (size_t)n_queries * 40, n_queries, hipGetErrorString(e));
    e = hipMemcpyAsync(f.d_q.get(), f.q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.d_nbb.get(), f.nbb.data(), sizeof(uint32_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(f.d_stat.get(), 0, sizeof(double) * 3 * (size_t)n_queries, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(f.d_free.get(), 0, sizeof(unsigned long long) * (size_t)n_queries, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (f's vectors are read until here)
    if (e != hipSuccess) return fail(h, BISBM_ERR_HIP, "bisbm_conditionals_set: %s", hipGetErrorString(e));
    h->cond = std::move(f);
    return BISBM_OK;
}

int bisbm_conditionals_set_reference(bisbm_handle h, const uint32_t* labels) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->cond.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    uint32_t ka = 0, kb = 0;
    if (labels) {  // (before anything changes)
        if (int rc = shared_shape(h, &ka, &kb)) return rc;
        if (any_wide(h))
            return fail(h, BISBM_ERR_UNSUPPORTED, "the soft marginals serve byte labels only (at most 256 blocks; this handle has %u + %u)", ka, kb);
        if (any_grouped(h)) return fail(h, BISBM_ERR_STATE, "the soft marginals need chains that are not grouped by shape");
        if (int rc = check_reference_labels(h, labels, ka, kb)) return rc;
    }
    if (!h->devs.empty())
        if (int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_conditionals_set_reference(d, labels); })) return rc;
    ConditionalState& s = h->cond;
    ++s.ref_serial;
    s.prob_terms = 0;
    if (!labels) {
        s.ref = AlignRef();
        if (h->devs.empty()) s.d_prob.reset(), s.prob_cells = 0;
        return BISBM_OK;
    }
    s.ref.labels.assign(labels, labels + h->n);
    s.ref.has = true, s.ref.chain = -1, s.ref.ka = ka, s.ref.kb = kb;
    if (!h->devs.empty()) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    s.prob_cells = (size_t)s.n * std::max(ka, kb);
    RESERVE(h, s.d_prob, s.prob_cells);
    if (int rc = zero_prob(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_conditionals_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    ConditionalState& s = h->cond;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "node conditionals serve byte labels only (at most 256 blocks): merge the blocks down first");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_conditionals_accumulate");
    if (s.ref.has) {
        uint32_t ka = 0, kb = 0;
        if (any_grouped(h) || shared_shape(h, &ka, &kb) != BISBM_OK)
            return fail(h, BISBM_ERR_STATE, "the reference partition of the soft marginals was set for %u + %u blocks, the chains are now grouped by shape: clear it or set it again",
                        s.ref.ka, s.ref.kb);
        if (s.ref.ka != ka || s.ref.kb != kb)
            return fail(h, BISBM_ERR_STATE, "the reference partition of the soft marginals was set for %u + %u blocks, the chains now have %u + %u: set it again", s.ref.ka,
                        s.ref.kb, ka, kb);
    }
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_conditionals_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    const bool keep = (s.what & BISBM_COND_KEEP_LAST) != 0;
    // the rows of this sample: one segment per leaf, chains in the leaf's order
    s.segments.clear();
    size_t total = 0;
    for (bisbm_engine* e : leaves(h)) {
        ConditionalState::Segment seg;
        seg.ka = e->ka, seg.kb = e->kb, seg.base = total;
        seg.chain.resize(e->n_chains);
        for (uint32_t c = 0; c < e->n_chains; ++c) seg.chain[c] = e == h ? c : e->ridx[c];
        total += (size_t)e->n_chains * row_total(s, e->ka, e->kb);
        s.segments.push_back(std::move(seg));
    }
    if (keep) {
        hipError_t err = s.d_dS.reserve(total);
        if (err == hipSuccess) err = s.d_P.reserve(total);
        if (err != hipSuccess) {
            s.segments.clear();
            return fail(h, BISBM_ERR_HIP, "bisbm_conditionals_accumulate: %zu bytes of device memory for the rows of one sample could not be allocated: %s",
                        2 * total * sizeof(double), hipGetErrorString(err));
        }
    }
    size_t i = 0;
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains, in group order)
        if (int rc = add_sample(h, e, s.segments[i++])) {
            s.segments.clear();
            return rc;
        }
    if (!keep) s.segments.clear();
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_conditionals_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_conditionals_reset(d); });
    ConditionalState& s = h->cond;
    s.terms = 0;
    s.segments.clear();
    if (!s.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(s.d_stat.get(), 0, sizeof(double) * 3 * (size_t)s.n, h->stream));
    HIPCHK(h, hipMemsetAsync(s.d_free.get(), 0, sizeof(unsigned long long) * (size_t)s.n, h->stream));
    if (int rc = zero_prob(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_conditionals_get_stats(bisbm_handle h, double* stay_sum, double* entropy_sum, double* margin_sum, uint64_t* free_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ConditionalState& s = h->cond;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    if (terms_out) {
        *terms_out = 0;
        for (bisbm_engine* d : entries) *terms_out += d->cond.terms;
    }
    DeviceGuard keep;
    std::vector<double> part(3 * (size_t)s.n);
    std::vector<unsigned long long> fpart(s.n);
    double* outs[3] = {stay_sum, entropy_sum, margin_sum};
    bool first = true;
    for (bisbm_engine* d : entries) {  // (several devices: the device sums are added on the host in device order)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        HIPCHK(h, hipMemcpy(part.data(), d->cond.d_stat.get(), sizeof(double) * part.size(), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(fpart.data(), d->cond.d_free.get(), sizeof(unsigned long long) * fpart.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k)
            if (outs[k])
                for (size_t i = 0; i < s.n; ++i) outs[k][i] = first ? part[k * (size_t)s.n + i] : outs[k][i] + part[k * (size_t)s.n + i];
        if (free_out)
            for (size_t i = 0; i < s.n; ++i) free_out[i] = (first ? 0 : free_out[i]) + fpart[i];
        first = false;
    }
    return BISBM_OK;
}

int bisbm_conditionals_get_marginals(bisbm_handle h, double* prob_out, uint32_t* kmax_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ConditionalState& s = h->cond;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (!s.ref.has) return fail(h, BISBM_ERR_STATE, "no reference partition: the soft marginals are kept after bisbm_conditionals_set_reference only");
    const std::vector<bisbm_engine*> entries = device_entries(h);
    const uint32_t kmax = std::max(s.ref.ka, s.ref.kb);
    if (kmax_out) *kmax_out = kmax;
    if (terms_out) {
        *terms_out = 0;
        for (bisbm_engine* d : entries) *terms_out += d->cond.prob_terms;
    }
    if (!prob_out) return BISBM_OK;
    const size_t cells = (size_t)s.n * kmax;
    DeviceGuard keep;
    std::vector<double> part(h->devs.empty() ? 0 : cells);
    bool first = true;
    for (bisbm_engine* d : entries) {
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        double* dst = h->devs.empty() ? prob_out : part.data();
        HIPCHK(h, hipMemcpy(dst, d->cond.d_prob.get(), sizeof(double) * cells, hipMemcpyDeviceToHost));
        if (!h->devs.empty())
            for (size_t i = 0; i < cells; ++i) prob_out[i] = first ? part[i] : prob_out[i] + part[i];
        first = false;
    }
    return BISBM_OK;
}

int bisbm_conditionals_get_last(bisbm_handle h, uint32_t query_index, uint32_t stride, double* dS_out, double* p_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ConditionalState& s = h->cond;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (!(s.what & BISBM_COND_KEEP_LAST))
        return fail(h, BISBM_ERR_STATE, "the last rows are not kept: bisbm_conditionals_set was called without BISBM_COND_KEEP_LAST");
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u queries are set", query_index, s.n);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    const bool tb = s.q[query_index] >= h->na;
    for (bisbm_engine* d : entries) {
        if (d->cond.segments.empty()) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_conditionals_accumulate before bisbm_conditionals_get_last");
        for (const ConditionalState::Segment& seg : d->cond.segments)
            if (stride < (tb ? seg.kb : seg.ka))
                return fail(h, BISBM_ERR_INVALID_ARG, "stride = %u: a chain has %u blocks of the query's type", stride, tb ? seg.kb : seg.ka);
    }
    DeviceGuard keep;
    std::vector<double> tmp;
    for (size_t di = 0; di < entries.size(); ++di) {
        bisbm_engine* d = entries[di];
        const ConditionalState& ds = d->cond;
        const uint32_t chain_base = h->devs.empty() ? 0u : h->dev_first[di], nbb = ds.nbb[query_index];
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        for (const ConditionalState::Segment& seg : ds.segments) {
            const size_t k_own = tb ? seg.kb : seg.ka, rt = row_total(ds, seg.ka, seg.kb);
            const size_t at = (size_t)(query_index - nbb) * seg.ka + (size_t)nbb * seg.kb;
            tmp.resize(seg.chain.size() * k_own);
            for (int which = 0; which < 2; ++which) {
                double* out = which ? p_out : dS_out;
                if (!out) continue;
                const double* src = (which ? ds.d_P.get() : ds.d_dS.get()) + seg.base + at;
                HIPCHK(h, hipMemcpy2D(tmp.data(), k_own * sizeof(double), src, rt * sizeof(double), k_own * sizeof(double), seg.chain.size(), hipMemcpyDeviceToHost));
                for (size_t c = 0; c < seg.chain.size(); ++c) {
                    double* row = out + (size_t)(chain_base + seg.chain[c]) * stride;
                    const bool counted = !std::isnan(tmp[c * k_own]);
                    for (size_t x = 0; x < stride; ++x)  // (a chain that was not counted: NaN over the whole row)
                        row[x] = !counted ? std::numeric_limits<double>::quiet_NaN() : x < k_own ? tmp[c * k_own + x] : 0.;
                }
            }
        }
    }
    return BISBM_OK;
}

int bisbm_debug_log(bisbm_handle h, const double* x, size_t count, double* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) {
        const int rc = bisbm_debug_log(h->devs[0], x, count, out);
        if (rc) h->err = h->devs[0]->err;
        return rc;
    }
    if (!x || !out) return fail(h, BISBM_ERR_INVALID_ARG, "NULL argument");
    if (count == 0) return BISBM_OK;
    DeviceGuard keep;
    HIPCHK(h, hipSetDevice(h->device));
    DeviceBuf<double> dx, dout;
    RESERVE(h, dx, count);
    RESERVE(h, dout, count);
    HIPCHK(h, hipMemcpy(dx.get(), x, sizeof(double) * count, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(log_probe_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (const double*)dx.get(), count, dout.get());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, dout.get(), sizeof(double) * count, hipMemcpyDeviceToHost));
    return BISBM_OK;
}

int bisbm_held_conditionals_set(bisbm_handle h, int on) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->cond.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    const bool held = on != 0;
    if (!h->devs.empty())
        if (int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_held_conditionals_set(d, on); })) return rc;
    if (h->cond.held == held) return BISBM_OK;  // (not a switch: the sums stay)
    h->cond.held = held;
    if (!h->devs.empty()) return BISBM_OK;
    return bisbm_conditionals_reset(h);  // a sum over two definitions means nothing: the sums, prob and the last rows go
}

int bisbm_held_conditionals_get(bisbm_handle h, int* on_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->cond.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (!on_out) return fail(h, BISBM_ERR_INVALID_ARG, "on_out is NULL");
    *on_out = h->cond.held ? 1 : 0;
    return BISBM_OK;
}

int bisbm_least_settled_topk(bisbm_handle h, uint32_t by, uint32_t k, uint32_t* query_out, double* value_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ConditionalState& s = h->cond;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "%s", kNoQueries);
    if (by != BISBM_SETTLED_BY_ENTROPY && by != BISBM_SETTLED_BY_STAY)
        return fail(h, BISBM_ERR_INVALID_ARG, "by = %u: BISBM_SETTLED_BY_ENTROPY (0) or BISBM_SETTLED_BY_STAY (1)", by);
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_least_settled_topk selects at most %u queries", k, kQueryMaxK);
    if (!query_out) return fail(h, BISBM_ERR_INVALID_ARG, "query_out is NULL");
    const uint64_t terms = total_terms(h, &bisbm_engine::cond);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_conditionals_accumulate before bisbm_least_settled_topk");
    if (terms_out) *terms_out = terms;
    // one row: the n entries of the statistic (d_stat holds stay, entropy, margin, n each), the candidates the query indices
    bisbm_engine* e = device_entries(h)[0];  // the device that selects
    ConditionalState& w = e->cond;
    const std::vector<uint64_t> off{0, s.n};
    {  // (24 bytes, written at every call)
        const TopkCand cand{0u, 0xffffffffu};
        DeviceGuard keep;
        HIPCHK(h, hipSetDevice(e->device));
        RESERVE(h, w.d_sel_off, 2);
        RESERVE(h, w.d_sel_cand, 1);
        HIPCHK(h, hipMemcpy(w.d_sel_off.get(), off.data(), sizeof(uint64_t) * 2, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(w.d_sel_cand.get(), &cand, sizeof(cand), hipMemcpyHostToDevice));
    }
    const size_t at = by == BISBM_SETTLED_BY_STAY ? 0 : (size_t)s.n;
    const auto stat_of = [at](bisbm_engine* d) { return (const double*)d->cond.d_stat.get() + at; };
    return topk_select(h, __func__, per_device(h, stat_of), off, w.topk, w.d_sel_off.get(), w.d_sel_cand.get(), nullptr, k, query_out, value_out,
                       by == BISBM_SETTLED_BY_STAY);
}

}  // extern "C"
