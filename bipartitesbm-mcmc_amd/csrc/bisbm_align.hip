// bisbm_align.hip -- label alignment of the chains before their samples are pooled into the marginal histogram
// (include/bisbm.h, "Label alignment before pooling").  A block label means something only inside one chain; per sample and
// per chain and node type this unit
//   1. counts the overlap table C[r][s] of the chain's labels with the reference partition (align_overlap_kernel),
//   2. finds the permutation of the chain's blocks that maximises the overlap, exactly (align_assign_kernel: one wavefront per
//      chain and type runs the shortest-augmenting-path assignment of bisbm_align_assignment below),
//   3. counts the chain's labels through that permutation (marginals_aligned_kernel: the marginals kernel of
//      bisbm_kernels.hip with the permutation rows staged in LDS).
// The chains' own state is only read.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr long long kInf = 0x3fffffffffffffffLL;

// ------------------------------------------------------------------------------------------
// 1. overlap tables: tab[c][ka*ka + kb*kb], type a at 0 (C[r][s] at r*ka + s), type b at ka*ka (r*kb + s), r = the chain's
// label, s = the reference's, both within the type.  Integer atomics: the tables do not depend on the order of the adds.
// ------------------------------------------------------------------------------------------
struct OverlapParams {
    const uint8_t* labels;  // [chain][label_stride]
    size_t label_stride;
    const uint8_t* ref;     // [label_stride] (n used)
    uint32_t n, na, ka, kb, nodes_per_block;
    uint32_t* tab;
};

enum TableMode { kTablePerWave = 0, kTablePerBlock = 1, kTableInHbm = 2 };

// kTablePerWave: a table per wave in LDS (an aligned chain sends most nodes of a wave to the K diagonal cells: the four waves
// do not queue on each other's cells), summed into HBM at the end; kTablePerBlock: one table in LDS; kTableInHbm: the table is
// too large for a useful occupancy, count straight into HBM.
template <int MODE>
__global__ __launch_bounds__(256) void align_overlap_kernel(OverlapParams p) {
    extern __shared__ __align__(16) uint32_t lds_tab[];
    const uint32_t c = blockIdx.y;
    const uint32_t T = p.ka * p.ka + p.kb * p.kb;
    uint32_t* out = p.tab + (size_t)c * T;
    uint32_t* t = MODE == kTableInHbm ? out : lds_tab + (MODE == kTablePerWave ? (threadIdx.x / 64) * T : 0);
    if constexpr (MODE != kTableInHbm) {
        const uint32_t tot = MODE == kTablePerWave ? 4 * T : T;
        for (uint32_t i = threadIdx.x; i < tot; i += 256) lds_tab[i] = 0;
        __syncthreads();
    }
    const uint8_t* lab = p.labels + (size_t)c * p.label_stride;
    const uint32_t v0 = blockIdx.x * p.nodes_per_block;  // (a multiple of 1024: the word loads below are aligned)
    const uint32_t v1 = min(p.n, v0 + p.nodes_per_block);
    for (uint32_t w = v0 + 4 * threadIdx.x; w < v1; w += 4 * 256) {
        // (w + 3 < label_stride: rows are padded to a multiple of 256 labels, the reference buffer is label_stride bytes)
        const uint32_t L = *(const uint32_t*)(lab + w);
        const uint32_t R = *(const uint32_t*)(p.ref + w);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = w + j;
            if (v >= v1) break;
            const bool tb = v >= p.na;
            const uint32_t base = tb ? p.ka : 0u, kt = tb ? p.kb : p.ka;
            const uint32_t r = ((L >> (8 * j)) & 0xffu) - base, s = ((R >> (8 * j)) & 0xffu) - base;
            if (r < kt && s < kt) atomicAdd(t + (tb ? p.ka * p.ka : 0u) + r * kt + s, 1u);
        }
    }
    if constexpr (MODE != kTableInHbm) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < T; i += 256) {
            uint32_t x = lds_tab[i];
            if (MODE == kTablePerWave) x += lds_tab[T + i] + lds_tab[2 * T + i] + lds_tab[3 * T + i];
            if (x) atomicAdd(out + i, x);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 2. assignment: one wavefront per (chain, type).  The solver of bisbm_align_assignment, 1-based as there: column 0 is the
// virtual start column, p[j] the row (1..K) assigned to column j.  Lane l owns columns 1 + l + 64 q (q < 4: K <= 255), their
// dual v, least reduced distance minv and visited bit in registers; the row duals u, p and the path links `way` are in LDS.
// The argmin of a Dijkstra step (least minv, ties -> lowest column) is a wave reduction.
// ------------------------------------------------------------------------------------------
struct AssignParams {
    const uint32_t* tab;
    uint32_t ka, kb;
    uint8_t* perm;   // [chain][ka + kb]
    uint64_t* tot;   // [chain][2]
};

constexpr int kColsPerLane = 4;

__global__ __launch_bounds__(64) void align_assign_kernel(AssignParams p) {
    __shared__ long long u[256];
    __shared__ uint32_t pr[256], way[256];
    const uint32_t c = blockIdx.x, type = blockIdx.y, lane = threadIdx.x;
    const uint32_t K = type ? p.kb : p.ka;
    const uint32_t* C = p.tab + (size_t)c * (p.ka * p.ka + p.kb * p.kb) + (type ? p.ka * p.ka : 0u);
    uint32_t mx = 0;
    for (uint32_t i = lane; i < K * K; i += 64) mx = max(mx, C[i]);
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    const long long cmax = mx;
    for (uint32_t i = lane; i <= K; i += 64) u[i] = 0, pr[i] = 0, way[i] = 0;
    long long v[kColsPerLane], minv[kColsPerLane];
#pragma unroll
    for (int q = 0; q < kColsPerLane; ++q) v[q] = 0;
    __syncthreads();
    for (uint32_t i = 1; i <= K; ++i) {
        if (lane == 0) pr[0] = i;
        uint32_t j0 = 0, used = 0;
#pragma unroll
        for (int q = 0; q < kColsPerLane; ++q) minv[q] = kInf;
        __syncthreads();
        while (true) {
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q)
                if (j0 == 1 + lane + 64 * q) used |= 1u << q;
            const uint32_t i0 = pr[j0];
            const long long ui0 = u[i0];
            const uint32_t* row = C + (size_t)(i0 - 1) * K;
            long long best = kInf;
            uint32_t bj = 0xffffffffu;
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q) {
                const uint32_t j = 1 + lane + 64 * q;
                if (j <= K && !((used >> q) & 1u)) {
                    const long long cur = cmax - (long long)row[j - 1] - ui0 - v[q];
                    if (cur < minv[q]) {
                        minv[q] = cur;
                        way[j] = j0;
                    }
                    if (minv[q] < best) best = minv[q], bj = j;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const long long ob = __shfl_xor(best, off);
                const uint32_t oj = (uint32_t)__shfl_xor((int)bj, off);
                if (ob < best || (ob == best && oj < bj)) best = ob, bj = oj;
            }
            __syncthreads();  // (every lane has read u[i0] before the duals move)
            if (lane == 0) u[pr[0]] += best;  // column 0 is visited from the start
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q) {
                const uint32_t j = 1 + lane + 64 * q;
                if (j <= K) {
                    if ((used >> q) & 1u) {
                        u[pr[j]] += best;
                        v[q] -= best;
                    } else {
                        minv[q] -= best;
                    }
                }
            }
            __syncthreads();
            j0 = bj;
            if (pr[j0] == 0) break;
        }
        if (lane == 0) {  // augment along the path
            do {
                const uint32_t j1 = way[j0];
                pr[j0] = pr[j1];
                j0 = j1;
            } while (j0);
        }
        __syncthreads();
    }
    const uint32_t base = type ? p.ka : 0u;
    uint8_t* perm = p.perm + (size_t)c * (p.ka + p.kb) + base;
    unsigned long long total = 0;
#pragma unroll
    for (int q = 0; q < kColsPerLane; ++q) {
        const uint32_t j = 1 + lane + 64 * q;
        if (j <= K) {
            const uint32_t r = pr[j] - 1;
            perm[r] = (uint8_t)(base + j - 1);
            total += C[(size_t)r * K + j - 1];
        }
    }
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0) p.tot[(size_t)c * 2 + type] = total;
}

// ------------------------------------------------------------------------------------------
// 3. the marginals kernel (bisbm_kernels.hip) counting perm[c][label] instead of label.  The permutation rows of kPermChunk
// chains at a time are staged in LDS behind the per-thread counter rows.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPermChunk = 64;

template <bool IN_LDS>
__global__ __launch_bounds__(256) void marginals_aligned_kernel(MarginalParams p, const uint8_t* perm, uint32_t K) {
    extern __shared__ __align__(16) uint32_t hist[];  // IN_LDS: one row of (kmax | 1) counters per thread; then the perm rows
    const uint32_t stride = p.kmax | 1u;
    uint8_t* pm = (uint8_t*)(hist + (IN_LDS ? 256 * stride : 0u));
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < p.n;
    const uint32_t base = v < p.na ? 0u : p.ka;
    uint32_t* row = IN_LDS ? hist + threadIdx.x * stride : p.counts + (size_t)v * p.kmax;
    if (IN_LDS)
        for (uint32_t j = 0; j < p.kmax; ++j) row[j] = 0;
    for (uint32_t c0 = 0; c0 < p.n_chains; c0 += kPermChunk) {
        const uint32_t nc = min(kPermChunk, p.n_chains - c0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nc * K; i += 256) pm[i] = perm[(size_t)c0 * K + i];
        __syncthreads();
        if (live)
            for (uint32_t c = 0; c < nc; ++c)
                if (!p.rung || p.rung[c0 + c] == 0u) row[(uint32_t)pm[c * K + p.labels[(size_t)(c0 + c) * p.label_stride + v]] - base] += 1;
    }
    if (IN_LDS && live) {
        uint32_t* out = p.counts + (size_t)v * p.kmax;
        for (uint32_t j = 0; j < p.kmax; ++j)
            if (row[j]) out[j] += row[j];
    }
}

}  // namespace

// Which overlap-table kernel serves a shape: the per-wave tables up to 64 KiB per workgroup (32 + 32 blocks: 32 KiB), one table
// per workgroup up to 64 KiB, HBM above.  BISBM_ALIGN_TABLE=wave|block|hbm forces a mode where it fits (tools/align_bench.py).
int bisbm::overlap_mode(uint32_t T) {
    const size_t limit = 64 * 1024;
    int mode = 4 * sizeof(uint32_t) * (size_t)T <= limit ? kTablePerWave : sizeof(uint32_t) * (size_t)T <= limit ? kTablePerBlock : kTableInHbm;
    if (const char* e = std::getenv("BISBM_ALIGN_TABLE")) {
        const int want = !strcmp(e, "wave") ? kTablePerWave : !strcmp(e, "block") ? kTablePerBlock : !strcmp(e, "hbm") ? kTableInHbm : -1;
        if (want >= mode) mode = want;
    }
    return mode;
}

// (shared with the mode-resolved marginals, bisbm_mode_marginals.hip, like overlap_mode)
hipError_t bisbm::launch_align_assign(const uint32_t* tab, uint32_t ka, uint32_t kb, uint8_t* perm, uint64_t* tot, uint32_t n_tables, hipStream_t stream) {
    AssignParams ap{};
    ap.tab = tab;
    ap.ka = ka;
    ap.kb = kb;
    ap.perm = perm;
    ap.tot = tot;
    hipLaunchKernelGGL(align_assign_kernel, dim3(n_tables, 2), dim3(64), 0, stream, ap);
    return hipGetLastError();
}

namespace {

hipError_t launch_overlap(const OverlapParams& p0, uint32_t n_chains, hipStream_t stream) {
    OverlapParams p = p0;
    const uint32_t T = p.ka * p.ka + p.kb * p.kb;
    // about 8192 workgroups over all chains, at least 4096 nodes each (the LDS tables are zeroed and summed once per workgroup)
    const uint32_t max_chunks = (p.n + 4095) / 4096;
    const uint32_t chunks = std::max(1u, std::min(max_chunks, (8192 + n_chains - 1) / n_chains));
    p.nodes_per_block = (((p.n + chunks - 1) / chunks) + 1023) & ~1023u;
    const dim3 grid((p.n + p.nodes_per_block - 1) / p.nodes_per_block, n_chains), block(256);
    switch (overlap_mode(T)) {
        case kTablePerWave:
            hipLaunchKernelGGL(align_overlap_kernel<kTablePerWave>, grid, block, 4 * sizeof(uint32_t) * T, stream, p);
            break;
        case kTablePerBlock:
            hipLaunchKernelGGL(align_overlap_kernel<kTablePerBlock>, grid, block, sizeof(uint32_t) * T, stream, p);
            break;
        default:
            hipLaunchKernelGGL(align_overlap_kernel<kTableInHbm>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_marginals_aligned(const MarginalParams& p, const uint8_t* perm, uint32_t K, hipStream_t stream) {
    const size_t pm = kPermChunk * K, hist = sizeof(uint32_t) * 256 * (p.kmax | 1u);
    const dim3 grid((p.n + 255) / 256), block(256);
    if (hist + pm > kLdsPerCu) {
        hipLaunchKernelGGL(marginals_aligned_kernel<false>, grid, block, pm, stream, p, perm, K);
        return hipGetLastError();
    }
    hipError_t e = hipFuncSetAttribute((const void*)marginals_aligned_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(hist + pm));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(marginals_aligned_kernel<true>, grid, block, hist + pm, stream, p, perm, K);
    return hipGetLastError();
}

// ---- host side --------------------------------------------------------------------------------------------------------

// one aligned sample of the chains of a kernel-running engine e into counts; `top` holds the reference
int align_leaf(bisbm_engine* e, const AlignState& top, uint32_t* counts) {
    AlignState& a = e->align;
    HIPCHK(e, hipSetDevice(e->device));
    const uint32_t ka = e->ka, kb = e->kb, K = ka + kb, C = e->n_chains;
    const size_t T = (size_t)ka * ka + (size_t)kb * kb;
    RESERVE(e, a.d_ref, e->label_stride);
    if (a.uploaded != top.serial) {
        std::vector<uint8_t> ref(e->label_stride, 0);
        for (uint64_t v = 0; v < e->n; ++v) ref[v] = (uint8_t)top.ref[v];
        HIPCHK(e, hipMemcpyAsync(a.d_ref.get(), ref.data(), ref.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        a.uploaded = top.serial;
    }
    a.have_perm = false;
    RESERVE(e, a.d_tab, C * T);
    RESERVE(e, a.d_perm, (size_t)C * K);
    RESERVE(e, a.d_tot, (size_t)C * 2);
    HIPCHK(e, hipMemsetAsync(a.d_tab.get(), 0, sizeof(uint32_t) * C * T, e->stream));
    OverlapParams op{};
    op.labels = e->d_labels;
    op.label_stride = e->label_stride;
    op.ref = a.d_ref.get();
    op.n = (uint32_t)e->n;
    op.na = (uint32_t)e->na;
    op.ka = ka;
    op.kb = kb;
    op.tab = a.d_tab.get();
    HIPCHK(e, launch_overlap(op, C, e->stream));
    HIPCHK(e, launch_align_assign(a.d_tab.get(), ka, kb, a.d_perm.get(), a.d_tot.get(), C, e->stream));
    MarginalParams mp{};
    mp.n = (uint32_t)e->n;
    mp.na = (uint32_t)e->na;
    mp.ka = ka;
    mp.kmax = std::max(ka, kb);
    mp.n_chains = C;
    mp.labels = e->d_labels;
    mp.label_stride = e->label_stride;
    mp.counts = counts;
    mp.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    HIPCHK(e, launch_marginals_aligned(mp, a.d_perm.get(), K, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    a.have_perm = true, a.perm_ka = ka, a.perm_kb = kb;
    return BISBM_OK;
}

// the library's reference: the labels of the lowest-description-length chain (ties -> the lowest global chain id, which is
// the lowest chain index of the handle); with replica exchange on, among the chains on rung 0
int pick_reference(bisbm_engine* h, uint32_t ka, uint32_t kb) {
    uint32_t n_chains = 0;
    if (int rc = bisbm_get_sizes(h, nullptr, nullptr, nullptr, &n_chains)) return rc;
    std::vector<double> S(n_chains);
    if (int rc = bisbm_entropy(h, S.data())) return rc;
    std::vector<uint32_t> rung(n_chains, 0);
    if (h->temper.L)
        if (int rc = bisbm_tempering_get(h, rung.data(), nullptr)) return rc;
    int64_t pick = -1;
    for (uint32_t c = 0; c < n_chains; ++c)
        if (rung[c] == 0u && (pick < 0 || S[c] < S[pick])) pick = c;
    const uint32_t best = (uint32_t)pick;  // (rung 0 holds n_chains / L >= 1 chains)
    std::vector<uint32_t> lab((size_t)h->n);
    if (int rc = bisbm_get_memberships(h, best, lab.data())) return rc;
    AlignState& a = h->align;
    a.ref.swap(lab);
    a.has_ref = true, a.ref_chain = best, a.ref_ka = ka, a.ref_kb = kb;
    ++a.serial;
    return BISBM_OK;
}

// the host solver (include/bisbm.h): the Jonker-Volgenant / Hungarian shortest-augmenting-path form, 1-based with column 0 as
// the virtual start; the device kernel above runs the same steps
void solve_assignment(uint32_t K, const uint32_t* C, uint32_t* perm, uint64_t* total) {
    long long cmax = 0;
    for (size_t i = 0; i < (size_t)K * K; ++i) cmax = std::max<long long>(cmax, C[i]);
    std::vector<long long> u(K + 1, 0), v(K + 1, 0), minv(K + 1);
    std::vector<uint32_t> p(K + 1, 0), way(K + 1, 0);
    std::vector<char> used(K + 1);
    for (uint32_t i = 1; i <= K; ++i) {
        p[0] = i;
        uint32_t j0 = 0;
        std::fill(minv.begin(), minv.end(), kInf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const uint32_t i0 = p[j0];
            long long delta = kInf;
            uint32_t j1 = 0;
            for (uint32_t j = 1; j <= K; ++j)
                if (!used[j]) {
                    const long long cur = cmax - (long long)C[(size_t)(i0 - 1) * K + j - 1] - u[i0] - v[j];
                    if (cur < minv[j]) minv[j] = cur, way[j] = j0;
                    if (minv[j] < delta) delta = minv[j], j1 = j;
                }
            for (uint32_t j = 0; j <= K; ++j)
                if (used[j])
                    u[p[j]] += delta, v[j] -= delta;
                else
                    minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const uint32_t j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    uint64_t tot = 0;
    for (uint32_t j = 1; j <= K; ++j) {
        perm[p[j] - 1] = j - 1;
        tot += C[(size_t)(p[j] - 1) * K + j - 1];
    }
    if (total) *total = tot;
}

}  // namespace

namespace bisbm {

int align_accumulate(bisbm_engine* h, uint32_t* device_counts) {
    if (!h->devs.empty() && device_counts)
        return fail(h, BISBM_ERR_UNSUPPORTED, "a handle over several devices accumulates into its own buffers (device_counts must be NULL); bisbm_marginals_map pools them");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "label alignment serves byte labels only (at most 256 blocks; this handle has %u + %u)", ka, kb);
    if (!device_counts) {
        // (as without the alignment: a histogram of other block counts is started afresh)
        bool stale = false;
        for (bisbm_engine* d : device_entries(h)) stale = stale || !d->d_counts || d->counts_cols != std::max(ka, kb);
        if (stale)
            if (int rc = bisbm_marginals_reset(h)) return rc;
    }
    AlignState& a = h->align;
    if (a.has_ref && (a.ref_ka != ka || a.ref_kb != kb)) {
        if (a.ref_chain < 0)
            return fail(h, BISBM_ERR_STATE, "the reference partition was set for %u + %u blocks, the chains now have %u + %u: set it again", a.ref_ka,
                        a.ref_kb, ka, kb);
        a.has_ref = false;
    }
    if (!a.has_ref)
        if (int rc = pick_reference(h, ka, kb)) return rc;
    // every leaf counts into the histogram of its device entry (a group's `root`), or into the caller's
    return each_leaf(h, [&](bisbm_engine* e) { return align_leaf(e, a, device_counts ? device_counts : (e->root ? e->root : e)->d_counts); });
}

}  // namespace bisbm

extern "C" {

int bisbm_marginals_set_alignment(bisbm_handle h, int mode) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (mode != BISBM_ALIGN_NONE && mode != BISBM_ALIGN_REFERENCE) return fail(h, BISBM_ERR_INVALID_ARG, "unknown alignment mode %d", mode);
    if (mode != h->align.mode && h->align.samples)
        return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples of the other alignment mode: bisbm_marginals_reset first");
    h->align.mode = mode;
    return BISBM_OK;
}

int bisbm_marginals_set_reference(bisbm_handle h, const uint32_t* labels) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_while_modes(h, "bisbm_marginals_set_reference", "bisbm_marginals_set_mode_reference")) return rc;
    AlignState& a = h->align;
    if (!labels) {
        a.has_ref = false;
        return BISBM_OK;
    }
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    for (uint64_t v = 0; v < h->n; ++v) {
        const bool tb = v >= h->na;
        if (labels[v] < (tb ? ka : 0u) || labels[v] >= (tb ? ka + kb : ka))
            return fail(h, BISBM_ERR_INVALID_ARG, "reference label %u of node %llu is outside its type's blocks [%u, %u)", labels[v],
                        (unsigned long long)v, tb ? ka : 0u, tb ? ka + kb : ka);
    }
    a.ref.assign(labels, labels + h->n);
    a.has_ref = true, a.ref_chain = -1, a.ref_ka = ka, a.ref_kb = kb;
    ++a.serial;
    return BISBM_OK;
}

int bisbm_marginals_get_reference(bisbm_handle h, uint32_t* labels_out, int64_t* chain_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_while_modes(h, "bisbm_marginals_get_reference", "bisbm_marginals_get_mode_reference")) return rc;
    const AlignState& a = h->align;
    if (!a.has_ref) return fail(h, BISBM_ERR_STATE, "no reference partition (none set, and no aligned sample since the last reset)");
    if (labels_out) std::copy(a.ref.begin(), a.ref.end(), labels_out);
    if (chain_out) *chain_out = a.ref_chain;
    return BISBM_OK;
}

int bisbm_marginals_get_alignment(bisbm_handle h, uint32_t chain, uint32_t* perm_out, uint64_t* overlap_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (chain >= h->n_chains) return fail(h, BISBM_ERR_INVALID_ARG, "chain %u out of range", chain);
    if (h->modes.n_modes) return mode_get_alignment(h, chain, perm_out, overlap_out);
    uint32_t local = 0;
    bisbm_engine* e = leaf_of_chain(h, chain, &local);
    const AlignState& a = e->align;
    if (!a.have_perm || a.perm_ka != e->ka || a.perm_kb != e->kb)
        return fail(h, BISBM_ERR_STATE, "chain %u has no aligned sample of its present block counts", chain);
    const uint32_t K = e->ka + e->kb;
    std::vector<uint8_t> perm(K);
    uint64_t tot[2];
    HIPCHK(h, hipSetDevice(e->device));
    HIPCHK(h, hipMemcpy(perm.data(), a.d_perm.get() + (size_t)local * K, K, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(tot, a.d_tot.get() + (size_t)local * 2, sizeof(tot), hipMemcpyDeviceToHost));
    if (perm_out)
        for (uint32_t r = 0; r < K; ++r) perm_out[r] = perm[r];
    if (overlap_out) *overlap_out = tot[0] + tot[1];
    return BISBM_OK;
}

int bisbm_align_assignment(uint32_t k, const uint32_t* table, uint32_t* perm_out, uint64_t* total_out) {
    if (k == 0 || !table || !perm_out) return fail(nullptr, BISBM_ERR_INVALID_ARG, "k must be >= 1, table and perm_out non-NULL");
    try {
        solve_assignment(k, table, perm_out, total_out);
    } catch (...) {
        return fail(nullptr, BISBM_ERR_INVALID_ARG, "out of host memory");
    }
    return BISBM_OK;
}

}  // extern "C"
